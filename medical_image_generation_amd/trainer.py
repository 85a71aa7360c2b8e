"""Fused DDPM train step on the HIP path (the hot loop of train_ldm.LDM.train_one_epoch, T-LDM:132-191, and of
train_ddpm.DDPM.train_one_epoch, T-DDPM:175-209):

    noise -> q-sample -> DiffusionModelUNet -> MSE -> backward -> (DDP all-reduce) -> clip_grad_norm_ -> Adam[W]

No torch autograd and no torch compute kernels in the step: the tape engine drives our kernels directly, the
optimizer is one fused launch over the flat parameter arena, and the whole step can be captured in a hipGraph
(`capture=True`) and replayed, which removes the Python / launch overhead of ~600 kernel launches.

`AETrainer` is the same thing for the generator step of train_autoencoder.AutoEncoder.train_one_epoch (T-AE:406-435):
encode -> sample -> decode -> L1 + kl_weight * KL (+ the native LPIPS-VGG term, `perceptual=`; + the caller's terms through `extra_loss`, evaluated by
torch autograd on the reconstruction: those networks are third-party torch modules) -> backward -> Adam.

Data parallelism: one process per GPU; the trainable prefix of the flat gradient arena is all-reduced
(average) over RCCL in a few large buckets -- statically unused `proj_attn.*` tensors live outside that prefix.

Validation (the loop that ends every epoch of the reference and decides `best_model.pth`: LDM.validate_epoch, train_ldm.py:193-239;
AutoEncoder.validate_one_epoch, train_autoencoder.py:438-467; adapt_kl_loss_weight, train_autoencoder.py:295-328): every trainer has
`validate()` / `capture_validate()` / `validate_graph()` -- the same forward without a tape, a forward-only loss reduction, and a
`ValidationMeter` that keeps the epoch's running mean on the device, so a validation epoch costs ONE host synchronisation
(`meter.mean()`, the number checkpoint.save_model takes as `validation_loss`: train_ldm.py:466-491, train_autoencoder.py:533-564).
Nothing the train step owns is written.

Averaged weights (`ema_decay=`; not in the reference): the optimizer launch also moves an exponential moving average of the trainable
parameters (`trainer.ema`), and `with trainer.ema_weights():` trades it with the parameters in place, so validation, sampling and
state_dict() read the average through the pointers they already hold.
"""
from __future__ import annotations

import contextlib
import math
import os

import torch
import torch.distributed as dist

from . import ddp
from . import engine as E
from . import hipops as ops
from . import inferer
from ._lib import call, call_raw, constants, ptr
from .optim import FusedAdam

F32 = torch.float32
METER_HEADER = constants()["MI_METER_HEADER"]  # {last batch loss, sum of batch losses, batch count, reserved}


class ValidationMeter:
    """Running mean of the per-batch validation losses, on the device: the `np.mean(losses)` of the reference's validation loops
    (train_ldm.py:231-239, train_autoencoder.py:458-461, 316-318) without a `.item()` per batch.

    `acc` is the fp64 block the mi_*_eval kernels update: acc[0] the last batch's loss, acc[1] the sum of the batch losses, acc[2] the
    number of batches (then the kernels' per-workgroup partials).  `last` is a device scalar (a view: the next batch overwrites it);
    `mean()` synchronises ONCE and returns a Python float.  With a process group of more than one rank, {sum, count} are all-reduced
    (SUM) first, so every rank gets the global mean -- ranks may have seen different numbers of batches.  On a CPU device only the
    reduction part works (`add()` stands in for the kernels): that is what the gloo tests drive."""

    def __init__(self, device, process_group=None):
        self.device = torch.device(device)
        self.pg = process_group
        n = call_raw("mi_meter_bytes") // 8 if self.device.type == "cuda" else METER_HEADER
        self.acc = torch.zeros(n, dtype=torch.float64, device=self.device)

    def reset(self):
        if self.acc.is_cuda:
            call("mi_meter_reset", ptr(self.acc))  # a kernel, like every write the captured graphs are ordered against
        else:
            self.acc[:METER_HEADER].zero_()

    def add(self, loss):
        """Account one batch loss computed elsewhere (a Python float or a tensor on the meter's device); no synchronisation."""
        loss = torch.as_tensor(loss, dtype=torch.float64, device=self.device).reshape(())
        self.acc[0] = loss
        self.acc[1] += loss
        self.acc[2] += 1.0

    @property
    def last(self):
        return self.acc[0]

    def mean(self) -> float:
        sc = self.acc[1:3]
        world = dist.get_world_size(self.pg) if (self.pg is not None or dist.is_initialized()) else 1
        if world > 1:
            sc = sc.clone()
            dist.all_reduce(sc, op=dist.ReduceOp.SUM, group=self.pg)
        total, count = sc.tolist()  # the one host synchronisation
        if count == 0:
            raise ValueError("ValidationMeter.mean(): no batch has been accounted since reset()")
        return total / count


def kl_weight_from_mean(kl_mean: float) -> float:
    """The decade rule of adapt_kl_loss_weight (train_autoencoder.py:319-327): kl_weight = 0.001 / 10 ** floor(log10(mean KL)), i.e.
    the weight that brings the KL term to the order of 1e-3 (3.7e3 -> 1e-6, 0.42 -> 1e-2, 1.0 -> 1e-3)."""
    kl_mean = float(kl_mean)
    if not kl_mean > 0 or math.isinf(kl_mean):
        raise ValueError(f"the mean KL must be positive and finite, got {kl_mean}")
    return 0.001 / 10.0 ** math.floor(math.log10(kl_mean))


def draw_drop(n, p, generator=None, device="cuda"):
    """A condition-dropout mask for classifier-free guidance training: torch.bool [n] on the device, True with probability p (Ho &
    Salimans 2022 train with p around 0.1 - 0.2).  `generator`: a torch generator of `device`.  Pass it as the trainers' `drop`."""
    if not 0.0 <= float(p) <= 1.0:
        raise ValueError(f"the drop probability must lie in [0, 1], got {p}")
    return torch.rand(int(n), device=device, generator=generator) < float(p)


class DDPMSchedule:
    """alphas_cumprod of generative's DDPMScheduler (closed form; see oracle/step.py for provenance)."""

    def __init__(self, num_train_timesteps=1000, schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0205,
                 prediction_type="epsilon", device="cuda"):
        betas = inferer.betas(schedule, num_train_timesteps, beta_start, beta_end)
        if prediction_type not in ("epsilon", "v_prediction"):
            raise ValueError(f"unknown prediction_type {prediction_type} (train_ldm.py:163-166 knows 'epsilon' and 'v_prediction')")
        acp = torch.cumprod(1.0 - betas, dim=0)
        self.num_train_timesteps, self.prediction_type = num_train_timesteps, prediction_type
        self.sqrt_acp = acp.sqrt().to(device)
        self.sqrt_1macp = (1.0 - acp).sqrt().to(device)


class _ArenaTrainer:
    """Optimizer state over the flat arena, gradient accumulation, data-parallel gradient exchange and hipGraph capture;
    subclasses give forward_backward().

    Data parallelism: the backward pass is cut ONCE, at the point where every gradient of the arena's *early* segment
    [arena.n_late, arena.n_trainable) is final (HipModule orders the arena so: the parameters whose gradients complete last -- the
    finest-resolution levels, conv_in and everything the time-embedding backward writes -- form the *late* prefix).  The SUM
    all-reduce of the early segment (>= 95 % of the bytes) is issued asynchronously at the cut and runs over xGMI while the rest of
    the backward (the full-resolution layers: ~1/3 of its time, almost no parameters) computes; the small late segment follows.
    The mean is never materialised: 1/world is folded into the optimizer kernel (`grad_scale`).

    overlap=False (or MI_DDP_OVERLAP=0) is the plain schedule: ONE backward (one hipGraph), then the all-reduce of the whole
    trainable prefix, then the optimizer -- the fallback should the overlapped exchange misbehave on a given RCCL / node (the N > 1
    overlap has been rehearsed with gloo ranks and with one-rank RCCL groups only: DESIGN.md section 6)."""

    def __init__(self, model, lr, optimizer, weight_decay, betas, eps, max_grad_norm, process_group, bucket_mb, device,
                 grad_accumulate_step=1, overlap=None, ema_decay=None, ema_warmup=False):
        self.model = model
        self.device = torch.device(device or "cuda")
        self.decoupled = optimizer == "AdamW"
        if optimizer not in ("AdamW", "Adam"):
            raise ValueError("optimizer must be 'Adam' or 'AdamW'")
        weight_decay = (0.01 if self.decoupled else 0.0) if weight_decay is None else weight_decay  # torch defaults
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if (process_group is not None or dist.is_initialized()) else 1
        self.bucket_elems = bucket_mb * (1 << 20) // 4
        if int(grad_accumulate_step) < 1:
            raise ValueError("grad_accumulate_step must be >= 1")
        self.grad_accumulate_step = int(grad_accumulate_step)
        self.arena = model.arena(self.device)
        if self.world > 1:
            ddp.broadcast_parameters(self.arena.data, 0, process_group)
        n = self.arena.n_trainable
        self.exp_avg = torch.zeros(n, dtype=F32, device=self.device)
        self.exp_avg_sq = torch.zeros(n, dtype=F32, device=self.device)
        self.step_count = torch.zeros(1, dtype=F32, device=self.device)
        # the torch.optim face of the fused optimizer: torch LR schedulers bind to it (train_ldm.py:124-130); lr / betas / eps /
        # weight_decay / max_grad_norm below are views of its parameter group
        # the shadow starts as a copy of the (broadcast) parameters, so the average needs no bias correction; ranks then stay identical
        # without a collective, because they apply identical updates
        self.ema = None if ema_decay is None else self.arena.data[:n].clone()
        self._ema_swapped = False  # inside ema_weights(): arena.data holds the average, self.ema the parameters
        self.optimizer = FusedAdam(model, self.arena, self.exp_avg, self.exp_avg_sq, self.step_count, lr, betas, eps, weight_decay,
                                   self.decoupled, max_grad_norm, 1.0 / self.world, ema=self.ema,
                                   ema_decay=0.0 if ema_decay is None else ema_decay, ema_warmup=ema_warmup)
        self.sumsq = self.optimizer.sumsq
        self.loss = torch.zeros(1, dtype=F32, device=self.device)
        self._accum = None       # fp32 [n_trainable]: sum of the gradients of the pending micro-steps (grad_accumulate_step > 1)
        self._micro = 0          # micro-steps since the last optimizer step
        self._graph = None
        self._static = None
        self._force_split = False  # tests: capture the two-graph form with world 1
        self._force_exchange = False  # tests: issue the (one-rank) collectives although world == 1
        self._val_meter = None   # the meter validate() uses when none is given
        self._val = None         # capture_validate(): (graph, static inputs, meter, outputs, pinned objects)
        self.overlap = (os.environ.get("MI_DDP_OVERLAP", "1") != "0") if overlap is None else bool(overlap)

    # ------------------------------------------------------------------ hyperparameters (self.optimizer's group)
    lr = property(lambda self: self.optimizer.lr, lambda self, v: setattr(self.optimizer, "lr", v))
    betas = property(lambda self: self.optimizer.betas, lambda self, v: setattr(self.optimizer, "betas", v))
    eps = property(lambda self: self.optimizer.eps, lambda self, v: setattr(self.optimizer, "eps", v))
    weight_decay = property(lambda self: self.optimizer.weight_decay, lambda self, v: setattr(self.optimizer, "weight_decay", v))

    @property
    def max_grad_norm(self):
        return self.optimizer.max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, v):
        self.optimizer.max_grad_norm = v

    # ------------------------------------------------------------------ averaged weights
    @property
    def ema_decay(self):
        """The decay of the shadow (None without one); like lr it may change between steps or replays."""
        return None if self.ema is None else self.optimizer.ema_decay

    @ema_decay.setter
    def ema_decay(self, v):
        if self.ema is None:
            raise RuntimeError("this trainer was built without ema_decay: whether a shadow exists is fixed at construction")
        self.optimizer.ema_decay = v

    ema_warmup = property(lambda self: self.optimizer.ema_warmup, lambda self, v: setattr(self.optimizer, "ema_warmup", bool(v)))

    def _need_ema(self):
        if self.ema is None:
            raise RuntimeError("this trainer keeps no averaged weights: construct it with ema_decay=")

    def _not_swapped(self, what):
        if self._ema_swapped:
            raise RuntimeError(f"{what} inside ema_weights(): the arena holds the averaged weights; leave the context first")

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context the arena's trainable prefix holds the averaged weights (and `trainer.ema` the parameters): one in-place
        exchange on entry and one on exit, so no pointer changes -- captured graphs, conv plans (they repack from the arena per run or
        replay), validate() / validate_graph(), inferer.sample() / invert() on trainer.model and model.state_dict() all read the
        average.  The statically unused tail is not touched.  Training calls and load_model are refused inside."""
        self._need_ema()
        self._not_swapped("ema_weights()")
        if self.model._arena is not self.arena:
            raise RuntimeError("the model's parameter arena was rebuilt after this trainer was created: the averaged weights belong to "
                               "the old buffers; create a new trainer")
        n = self.arena.n_trainable
        call("mi_swap_f32", ptr(self.arena.data), ptr(self.ema), n)
        self._ema_swapped = True
        try:
            yield self
        finally:
            call("mi_swap_f32", ptr(self.arena.data), ptr(self.ema), n)
            self._ema_swapped = False

    def ema_state_dict(self):
        """The network's state_dict() (names, shapes; CPU tensors) with every trainable tensor taken from the shadow; tensors that
        never receive a gradient and buffers come from the network.  No exchange: usable at any time."""
        self._need_ema()
        a = self.arena
        flat = (self.ema if not self._ema_swapped else a.data[:a.n_trainable]).detach().cpu()
        trainable = {n for n, _, t in self.model._entries if t}
        return {k: (a.view(k, flat).clone() if k in trainable else v.detach().cpu().clone()) for k, v in self.model.state_dict().items()}

    def load_ema_state_dict(self, sd):
        """Restore the shadow from an ema_state_dict(), in place (a captured optimizer graph keeps pointing at it)."""
        self._need_ema()
        self._not_swapped("load_ema_state_dict()")
        a = self.arena
        flat = self.ema.detach().cpu()
        for name, shape, t in self.model._entries:
            if t:
                if name not in sd or tuple(sd[name].shape) != tuple(shape):
                    raise ValueError(f"averaged weights: {name} is missing or has another shape than {tuple(shape)}")
                a.view(name, flat).copy_(sd[name].to(F32))
        self.ema.copy_(flat)

    def reset_ema(self):
        """shadow := current parameters."""
        self._need_ema()
        self._not_swapped("reset_ema()")
        self.ema.copy_(self.arena.data[:self.arena.n_trainable])

    # ------------------------------------------------------------------ pieces
    def _forward(self, *inputs):
        """-> (tape, out, dout): the network forward and the loss gradient at its output (subclasses)."""
        raise NotImplementedError

    def _fb_begin(self, *inputs):
        """Forward + the backward up to the model's cut mark (engine.CUT; the whole backward when nothing was marked).  Returns the
        state _fb_finish needs; it also keeps every tensor that is live across the cut alive, so the two halves can be captured
        into two hipGraphs sharing one memory pool."""
        tape, out, dout = self._forward(*inputs)
        tape.put(out, dout)
        fns, tape.fns = tape.fns, []
        i = len(fns)
        while i > 0:
            i -= 1
            if fns[i] is E.CUT:
                break
            fns[i]()
        return tape, fns[:i]

    def _fb_finish(self, state):
        tape, rest = state
        for fn in reversed(rest):
            fn()  # (a second CUT mark is a no-op)
        tape.grads.clear(), tape.keep.clear()

    def forward_backward(self, *inputs, on_cut=None):
        """Fresh gradients of one (micro-)batch into arena.grad, loss into self.loss.  on_cut(): called where every gradient of the
        arena's early segment [n_late, n_trainable) is final (data-parallel overlap)."""
        state = self._fb_begin(*inputs)
        if on_cut is not None:
            on_cut()
        self._fb_finish(state)

    def _exchanging(self):
        return self.world > 1 or self._force_exchange

    def _exchange(self):
        return ddp.GradientExchange(self.arena.grad, self.arena.n_late, self.arena.n_trainable, self.pg, self.bucket_elems,
                                    force=self._force_exchange)

    def all_reduce_grads(self):
        """SUM all-reduce of the whole trainable gradient prefix, no overlap (the mean is taken by the optimizer's grad_scale)."""
        if self._exchanging():
            self._exchange().finish()

    def optimizer_step(self):
        """clip_grad_norm_ + Adam[W] over the arena (self.optimizer.step(): pushes changed hyperparameters, then launches)."""
        self._not_swapped("optimizer_step()")
        self.optimizer.step()

    @staticmethod
    def _check_clip(opt, captured):
        if opt.clip != captured:
            raise RuntimeError("max_grad_norm was switched on or off after capture(): the captured graph "
                               f"{'computes' if captured else 'has no'} gradient norm; capture again")

    # ------------------------------------------------------------------ gradient accumulation (T-LDM:173-180, T-AE:389-397)
    def _fold_micro_step(self, boundary):
        """The reference sums the micro-step gradients (loss NOT divided) and clips / steps / zeroes on the boundary.  Every
        forward_backward() writes a fresh gradient into arena.grad; pending micro-steps live in a side buffer, so kernels that
        COPY gradients between tensors (a shortcut conv's bias gradient) never see stale sums."""
        n = self.arena.n_trainable
        if not boundary:
            if self._accum is None:
                self._accum = torch.empty(n, dtype=F32, device=self.device)
                call("mi_zero_f32_2d", ptr(self._accum), n, 1, n)
            call("mi_axpy_f32", ptr(self._accum), ptr(self.arena.grad), 1.0, n)
            self._micro += 1
            return
        if self._micro:
            call("mi_axpy_f32", ptr(self.arena.grad), ptr(self._accum), 1.0, n)
            call("mi_zero_f32_2d", ptr(self._accum), n, 1, n)
        self._micro = 0

    # ------------------------------------------------------------------ one step
    def step(self, *inputs, last_in_epoch=False):
        """One (micro-)step, eager; returns the (device) loss tensor of this micro-batch without synchronising.  With
        grad_accumulate_step = k the optimizer runs on every k-th call (or when last_in_epoch, T-LDM:173); the data-parallel
        exchange happens on that boundary micro-step only."""
        self._not_swapped("step()")
        boundary = (self._micro + 1) % self.grad_accumulate_step == 0 or last_in_epoch
        ex = self._exchange() if self._exchanging() and boundary else None
        # the early segment may leave at the cut only when no pending micro-step sum has to be folded in first
        self.forward_backward(*inputs, on_cut=ex.start_early if ex is not None and self._micro == 0 and self.overlap else None)
        self._fold_micro_step(boundary)
        if not boundary:
            return self.loss
        if ex is not None:
            ex.finish()
        self.optimizer_step()
        return self.loss

    def capture(self, *inputs, warmup=2):
        """Capture the step as hipGraphs around static input buffers; call step_graph() afterwards.  Graphs: forward + the backward up
        to the cut, the rest of the backward (only when there is something to overlap: world > 1), the optimizer.  RCCL is never
        inside a capture: the all-reduces are issued between the replays, the early segment's concurrently with the second graph."""
        self._not_swapped("capture()")
        if self.grad_accumulate_step != 1:
            raise RuntimeError("hipGraph capture covers grad_accumulate_step == 1; use step() for accumulation")
        static = tuple(None if t is None else t.clone() for t in inputs)  # (None: an optional input that is not used)
        self._warm_up(lambda: self.forward_backward(*static), warmup)
        self._static = static  # (bound once the warm-up has accepted the inputs: a refused capture() leaves an earlier one intact)
        split = self.overlap and (self.world > 1 or self._force_split) and 0 < self.arena.n_late < self.arena.n_trainable
        # thread_local: a collective library's watchdog thread polling events must not invalidate the capture
        self._g_fb, self._g_fb2 = torch.cuda.CUDAGraph(), None
        if not split:
            with torch.cuda.graph(self._g_fb, capture_error_mode="thread_local"):
                self.forward_backward(*self._static)
        else:
            with torch.cuda.graph(self._g_fb, capture_error_mode="thread_local"):
                state = self._fb_begin(*self._static)
            self._g_fb2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._g_fb2, pool=self._g_fb.pool(), capture_error_mode="thread_local"):
                self._fb_finish(state)
            del state
        self.optimizer.push()  # the graph reads the hyperparameters from the device block; step_graph() keeps it current
        self._clip_captured = self.optimizer.clip
        self._g_opt = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._g_opt, capture_error_mode="thread_local"):
            self.optimizer.launch()
        self._graph = True
        # The graphs hold raw device pointers of objects Python owns: the PackBatch (group tables), every conv plan (packed weights,
        # split slabs), the GroupNorm workspace and the arena.  Pin them for as long as the graphs exist -- a forward at another
        # shape between train steps (validation, DiffusionInferer.sample) replaces model._packb / grows the workspace, and their
        # destructors would hipFree memory the next replay still writes to.
        self._pinned = self._pin_state()

    @staticmethod
    def _warm_up(fn, passes):
        """`passes` runs of fn() on a side stream before a capture: they create the conv plans / workspaces (hipMalloc) outside it."""
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(passes):
                fn()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()

    def _load_static(self, static, inputs, where, remedy="capture again"):
        """Before a replay of the graphs captured by `where`: inputs given (None = keep) are copied into their static buffers."""
        if self.model._arena is not self.arena:  # .to() / .cuda() / load into new storage: the graphs point at the old buffers
            raise RuntimeError(f"the model's parameter arena was rebuilt after {where}: {remedy}")
        for buf, t in zip(static, inputs):
            if t is not None:
                if buf is None:
                    raise ValueError(f"this input was None at {where}: capture again with a tensor in its place")
                buf.copy_(t)

    def _pin_state(self):
        return [(m._packb, dict(m._plans), m._arena) for m in self._models()] + [dict(ops._ws_cache)]

    def _models(self):
        return [self.model]

    # ------------------------------------------------------------------ validation (T-LDM:193-239, T-AE:438-467, 295-328)
    def _eval_forward(self, meter, *inputs, **options):
        """The no-grad forward of one validation batch and its loss into `meter` (subclasses); returns extra outputs or None."""
        raise NotImplementedError

    def _meter(self, meter):
        if meter is None:
            if self._val_meter is None:
                self._val_meter = ValidationMeter(self.device, self.pg)
            meter = self._val_meter
        if not isinstance(meter, ValidationMeter) or meter.acc.device.type != self.device.type:
            raise ValueError("meter must be a ValidationMeter on the trainer's device")
        return meter

    def validate(self, *inputs, meter=None, **options):
        """One validation batch, eager and tape-less; the batch loss goes into `meter` (default: the trainer's own) and is returned as a
        device scalar (`meter.last`: fp64, overwritten by the next batch) without synchronising.  Takes step()'s inputs.  Writes nothing
        the train step owns: parameters, gradients, pending micro-step sums, moments, step count and `loss` stay bit-identical."""
        meter = self._meter(meter)
        extra = self._eval_forward(meter, *inputs, **options)
        return meter.last if extra is None else (meter.last, extra)

    def capture_validate(self, *inputs, warmup=1, meter=None, **options):
        """Capture validate() as ONE hipGraph around static copies of `inputs` -- independent of capture(): own graph, own memory pool,
        any batch size or patch shape.  The weight packing is inside the graph (the parameters change between epochs).  `meter` (default:
        the trainer's own) is a static pointer of the graph.  The warm-up passes (they create the conv plans and workspaces of this
        shape outside the capture) run on a scratch meter, so `meter` is not touched before the first validate_graph()."""
        meter = self._meter(meter)
        scratch = {k: (ValidationMeter(self.device) if isinstance(v, ValidationMeter) else v) for k, v in options.items()}
        static = tuple(None if t is None else t.clone() for t in inputs)
        self._warm_up(lambda: self._eval_forward(ValidationMeter(self.device), *static, **scratch), max(1, warmup))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            extra = self._eval_forward(meter, *static, **options)
        # the pinning rule of capture(), in both directions: this graph keeps what it points at alive (so a later capture() / step at
        # another shape may replace the model's PackBatch or grow the workspace), and capture() keeps its own set (so this capture may)
        self._val = (g, static, meter, extra, self._pin_state() + [options])

    def validate_graph(self, *inputs, meter=None):
        """Replay; inputs given (positionally, None = keep) are copied into the static buffers first.  `meter`, when given, must be the
        one the graph was captured with.  Returns what validate() returns (extra outputs live in static buffers of the graph)."""
        if self._val is None:
            raise RuntimeError("call capture_validate() first")
        g, static, captured, extra, _ = self._val
        if meter is not None and meter is not captured:
            raise ValueError("validate_graph() accounts into the meter given to capture_validate(): its block is a static pointer of the graph")
        self._load_static(static, inputs, "capture_validate()")
        g.replay()
        return captured.last if extra is None else (captured.last, extra)

    def step_graph(self, *inputs):
        """Replay; inputs given (positionally, None = keep) are copied into the static buffers first."""
        self._not_swapped("step_graph()")
        assert self._graph, "call capture() first"
        self._load_static(self._static, inputs, "capture()", "create a new trainer (or call capture() again)")
        ex = self._exchange() if self._exchanging() else None
        self._g_fb.replay()
        if self._g_fb2 is not None:
            if ex is not None:
                ex.start_early()   # early segment: final once the first graph is done ...
            self._g_fb2.replay()   # ... and its all-reduce runs over xGMI while the rest of the backward computes
        if ex is not None:
            ex.finish()
        self._check_clip(self.optimizer, self._clip_captured)
        self.optimizer.step(replay=self._g_opt)  # block refreshed first: a scheduler / load_model between replays takes effect
        return self.loss


class DDPMTrainer(_ArenaTrainer):
    """step(x0, noise, timesteps[, class_labels][, context=...][, condition=...][, drop=...]): x0/noise fp32 NCDHW, timesteps (and class_labels)
    int64 [N]; context: fp32 [N, tokens, cross_attention_dim] for a net built with with_conditioning=True (the `context=` of
    DiffusionModelUNet.forward, UNet:1936-1944), a constant of the step like in forward().

    condition: channel-concatenation conditioning (the third-party inferer's `condition=..., mode="concat"`, the arguments of the call at
    train_ddpm.py:191; BASELINE configs[4] "label-channel conditioning"): fp32 NC'[D]HW, spatially like x0.  Only x0's channels are
    noised; the condition channels are written un-noised behind them -- model input = cat([noisy, condition], dim=1) with
    in_channels = C + C' -- and the model predicts x0's C channels (out_channels = C), compared with x0's noise.

    drop: condition dropout, the training half of classifier-free guidance (Ho & Salimans 2022; not part of the reference: PARITY
    UNPINNED) -- torch.bool or torch.uint8 [N] on the device (`draw_drop`), non-zero = this sample trains unconditionally.  One mask drops
    every conditioning the sample has, inside the step's kernels: its label becomes `null_class` (a row of the class embedding kept for
    "no class", given to the constructor; forward and backward use it, so dropped samples train that row), its context rows and its
    condition channels become zeros.  Like every input it is a static buffer of capture(): a new mask per replay needs no re-capture."""

    def __init__(self, model, lr=2e-5, optimizer="AdamW", weight_decay=None, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=1.0,
                 schedule: DDPMSchedule | None = None, process_group=None, bucket_mb=64, device=None, grad_accumulate_step=1, overlap=None,
                 ema_decay=None, ema_warmup=False, null_class=None):
        super().__init__(model, lr, optimizer, weight_decay, betas, eps, max_grad_norm, process_group, bucket_mb, device,
                         grad_accumulate_step, overlap, ema_decay, ema_warmup)
        self.schedule = schedule or DDPMSchedule(device=self.device)
        nce = getattr(model, "num_class_embeds", None)
        if null_class is not None and (nce is None or not 0 <= int(null_class) < nce):
            raise ValueError(f"null_class must be an index into the model's class embedding ([0, {nce})), got {null_class}"
                             if nce is not None else "null_class is for a model with num_class_embeds")
        self.null_class = None if null_class is None else int(null_class)

    def _check_inputs(self, x0, noise, timesteps, class_labels, context, condition, drop=None):
        """Raw pointers go to the kernels: refuse anything they would misread instead of reading out of bounds.  -> channels of `condition`."""
        m = self.model
        if not (x0.is_cuda and noise.is_cuda and timesteps.is_cuda):
            raise RuntimeError("DDPMTrainer inputs must live on the GPU")
        if x0.dtype != F32 or noise.dtype != F32 or not x0.is_contiguous() or not noise.is_contiguous() or x0.shape != noise.shape:
            raise ValueError("x0 and noise must be contiguous fp32 tensors of the same NC[D]HW shape")
        if timesteps.dtype != torch.int64 or timesteps.shape != (x0.shape[0],) or not timesteps.is_contiguous():
            raise ValueError("timesteps must be a contiguous int64 tensor of shape [N]")  # range: clamped to the schedule in k_qsample
        cc = 0
        if condition is not None:
            if not condition.is_cuda or condition.dtype != F32 or not condition.is_contiguous() or condition.dim() != x0.dim() or \
                    condition.shape[0] != x0.shape[0] or condition.shape[2:] != x0.shape[2:]:
                raise ValueError("condition must be a contiguous fp32 GPU tensor with x0's batch and spatial shape (mode='concat')")
            cc = condition.shape[1]
        if x0.shape[1] + cc != m.in_channels:
            raise ValueError(f"Input number of channels ({x0.shape[1] + cc}) is not equal to expected number of channels ({m.in_channels})")
        if x0.shape[1] != m.out_channels:  # the MSE compares the prediction with x0's noise channel for channel
            raise ValueError(f"the model predicts {m.out_channels} channels but the noised input has {x0.shape[1]}: the loss target "
                             "(the noise / velocity of x0) must have the prediction's channel count; un-noised conditioning channels go in "
                             "`condition=`")
        if (class_labels is None) != (getattr(m, "num_class_embeds", None) is None):
            raise ValueError("class_labels should be provided exactly when the model has num_class_embeds")
        if (context is not None) != bool(getattr(m, "with_conditioning", False)):
            raise ValueError("context should be provided exactly when the model has with_conditioning = True")
        if context is not None:
            if not context.is_cuda or context.dtype != F32 or context.dim() != 3 or context.shape[0] != x0.shape[0] or \
                    context.shape[2] != m.cross_attention_dim:
                raise ValueError(f"context must be a GPU fp32 tensor [batch, tokens, {m.cross_attention_dim}]")
        self._check_drop(drop, x0, class_labels, context, condition)
        return cc

    def _check_drop(self, drop, x0, class_labels, context, condition):
        """The condition-dropout mask against the batch (x0: any input that has the batch size and the device) and the conditioning."""
        if drop is None:
            return
        if not isinstance(drop, torch.Tensor) or drop.dtype not in (torch.bool, torch.uint8):
            raise ValueError("drop must be a torch.bool or torch.uint8 tensor (draw_drop)")
        if drop.shape != (x0.shape[0],) or not drop.is_contiguous():
            raise ValueError("drop must be a contiguous tensor of shape [N]")
        if drop.device != x0.device:
            raise ValueError("drop must live on the inputs' device")
        if class_labels is None and context is None and condition is None:
            raise ValueError("drop: this step has no conditioning to drop (no class_labels, context or condition)")
        if class_labels is not None:
            if self.null_class is None:
                raise ValueError("drop on a class-conditional model needs the trainer's null_class=: the label dropped samples train")
            if not class_labels.is_cuda or class_labels.dtype != torch.int64 or class_labels.shape != (x0.shape[0],) or \
                    not class_labels.is_contiguous():  # mi_select_labels reads it raw
                raise ValueError("class_labels must be a contiguous int64 GPU tensor of shape [N]")

    def _predict(self, grad_enabled, x0, noise, timesteps, class_labels, context, condition, cc, drop=None):
        """q-sample -> UNet.  -> (ctx, pred, target, (n, v), the tensors its kernels read); target: the noise, or the velocity mi_qsample
        wrote (v-prediction).  drop: the checked condition-dropout mask or None (then exactly the launches of a step without one)."""
        m = self.model
        sd = m.spatial_dims
        n, c = x0.shape[0], x0.shape[1]
        sp = tuple(x0.shape[2:])
        v = math.prod(sp)
        dims = (1,) * (3 - sd) + sp
        x_t = torch.empty((n,) + dims + (c + cc,), dtype=torch.bfloat16, device=x0.device)
        vpred = self.schedule.prediction_type == "v_prediction"  # target = scheduler.get_velocity(x0, noise, t), T-LDM:163-165
        target = torch.empty_like(noise) if vpred else noise
        mask = None if drop is None else drop.view(torch.uint8)  # (bool and uint8 share the byte layout the kernels read)
        qargs = (ptr(x0), ptr(noise), ptr(self.schedule.sqrt_acp), ptr(self.schedule.sqrt_1macp), ptr(timesteps), ptr(condition), cc,
                 ptr(x_t), ptr(target) if vpred else None, n, c, v, self.schedule.num_train_timesteps)
        if mask is None or not cc:
            call("mi_qsample", *qargs)
        else:
            call("mi_qsample_drop", *qargs, ptr(mask))  # zero condition channels for dropped samples
        ctx = E.Ctx(self.arena, m._plans, grad_enabled=grad_enabled, prepacked=m.pack_all())
        ctx_tokens = None
        if context is not None:
            context = context.contiguous()
            if mask is None:
                ctx_tokens = ops.cast_bf16(context.reshape(-1, context.shape[2]))
            else:  # zero context rows for dropped samples
                ctx_tokens = torch.empty((n * context.shape[1], context.shape[2]), dtype=torch.bfloat16, device=context.device)
                call("mi_cast_bf16_drop", ptr(context), ptr(ctx_tokens), ptr(mask), n, context.shape[1] * context.shape[2])
        if mask is not None and class_labels is not None:  # the effective labels: the embedding and its backward both read these
            labels = torch.empty_like(class_labels)
            call("mi_select_labels", ptr(class_labels), ptr(mask), self.null_class, ptr(labels), n)
            class_labels = labels
        pred = m._run(ctx, x_t, timesteps, need_dx=False, class_labels=class_labels, context=ctx_tokens)
        if pred.shape[-1] != target.shape[1]:  # k_mse indexes both with ONE channel count
            raise ValueError(f"prediction has {pred.shape[-1]} channels, the target {target.shape[1]}")
        return ctx, pred, target, (n, v), (x_t, target, ctx_tokens, condition, class_labels, mask)

    def _forward(self, x0, noise, timesteps, class_labels=None, context=None, condition=None, drop=None):
        """q-sample -> UNet -> MSE (+ its gradient).  x0/noise: fp32 NCDHW, timesteps: int64 [N]; class_labels: int64 [N], only for
        a net built with num_class_embeds; context: fp32 [N, tokens, cross_attention_dim], only for with_conditioning=True;
        condition: fp32 NC'[D]HW concatenated un-noised behind the noised channels (mode="concat"); drop: bool / uint8 [N], the
        samples that train without their conditioning (class docstring)."""
        cc = self._check_inputs(x0, noise, timesteps, class_labels, context, condition, drop)
        self.arena.grad.zero_()
        ctx, pred, target, (n, v), keep = self._predict(True, x0, noise, timesteps, class_labels, context, condition, cc, drop)
        dpred = torch.empty_like(pred)
        call("mi_mse_fwd_bwd", ptr(pred), ptr(target), ptr(dpred), ptr(self.loss), n, pred.shape[-1], v, 1.0)
        self._keep = keep  # read by kernels still in flight / by the second graph of a split capture
        return ctx.tape, pred, dpred

    def _eval_forward(self, meter, x0, noise, timesteps, class_labels=None, context=None, condition=None, drop=None):
        """LDM.validate_epoch's batch (T-LDM:206-229): q-sample -> UNet -> mse_loss against the noise / velocity; _forward's inputs and
        checks, no tape, no gradient tensor."""
        cc = self._check_inputs(x0, noise, timesteps, class_labels, context, condition, drop)
        _, pred, target, (n, v), _ = self._predict(False, x0, noise, timesteps, class_labels, context, condition, cc, drop)
        call("mi_mse_eval", ptr(pred), ptr(target), ptr(meter.acc), n, pred.shape[-1], v)


def _encode_sample(ae, arena, images, eps, grad_enabled, loss, kl_weight):
    """encode -> z = z_mu + eps * z_sigma (AEKL:786-787), channels-last: the head of the autoencoder's train step, of its validation
    batch and of the latent-diffusion trainer's frozen encoder.  Raw pointers go to the kernels: refuse anything they would misread
    instead of reading out of bounds (tensor metadata only: no synchronisation).  `loss`: the device scalar that is reset and then
    receives kl_weight * KL, or None -- reset only here, so a refused call leaves the last step's loss standing.  -> (ctx, x_cl, mu, sigma, z, (n, latent channels, latent voxels))."""
    if not (images.is_cuda and eps.is_cuda):
        raise RuntimeError("AETrainer inputs must live on the GPU")
    if images.dtype != F32 or not images.is_contiguous() or eps.dtype != F32 or not eps.is_contiguous():
        raise ValueError("images and eps must be contiguous fp32 GPU tensors")
    if images.dim() != ae.spatial_dims + 2 or images.shape[1] != ae.in_channels:
        raise ValueError(f"images must be NC[D]HW with {ae.in_channels} channels, got {tuple(images.shape)}")
    x_cl = ops.to_channels_last(images)
    ctx = E.Ctx(arena, ae._plans, grad_enabled=grad_enabled, prepacked=ae.pack_all())
    mu, sigma = ae._encode_run(ctx, x_cl, need_dx=False)
    n, lc = mu.shape[0], mu.shape[-1]
    lv = mu.numel() // (n * lc)
    if tuple(eps.shape) != (n, lc) + tuple(mu.shape[1:4])[3 - ae.spatial_dims:]:
        raise ValueError(f"eps must have the latent shape, got {tuple(eps.shape)}")
    if loss is not None:
        loss.zero_()
    z = torch.empty_like(mu)
    call("mi_reparam_kl_fwd", ptr(mu), ptr(sigma), ptr(eps), ptr(z), ptr(loss), n, lc, lv, kl_weight)
    return ctx, x_cl, mu, sigma, z, (n, lc, lv)


class LDMTrainer(DDPMTrainer):
    """The latent-diffusion train step as train_ldm.LDM.train_one_epoch runs it (T-LDM:145-180, 'vae' branch):

        latents = autoencoder.encode_stage_2_inputs(images)   (no grad: T-LDM:154-156)  ->  * scale_factor  ->  q-sample -> UNet
        -> MSE -> backward -> clip -> AdamW

    step(images, eps, noise, timesteps[, class_labels][, context=][, condition=][, drop=]): images fp32 NC[D]HW; eps fp32, latent-shaped -- the torch.randn_like of
    AutoencoderKL.sampling (AEKL:786-787) made an input so that a captured graph sees fresh noise and tests can pin it; noise fp32,
    latent-shaped (T-LDM:159); timesteps int64 [N].  The encoder runs tape-less on the same HIP kernels inside the same hipGraph.
    `scale_factor`: 1 / std of the first batch's latents (T-LDM:110-112) -- `estimate_scale_factor` -- or given."""

    def __init__(self, model, autoencoder, scale_factor: float | None = None, latent_space_type: str | None = None, **kw):
        from .vqvae import VQVAE
        is_vq = isinstance(autoencoder, VQVAE)
        if latent_space_type is None:
            latent_space_type = "vq" if is_vq else "vae"
        if latent_space_type not in ("vae", "vq"):
            raise ValueError("latent_space_type must be 'vae' or 'vq' (train_ldm.py -l)")
        if (latent_space_type == "vq") != is_vq:
            raise TypeError(f"latent_space_type={latent_space_type!r} with a {type(autoencoder).__name__}: 'vq' takes a VQVAE, 'vae' an AutoencoderKL")
        super().__init__(model, **kw)
        self.autoencoder = autoencoder
        self.latent_space_type = latent_space_type
        self.ae_arena = autoencoder.arena(self.device)
        self.scale_factor = None if scale_factor is None else float(scale_factor)
        if is_vq:  # x0 = 2 (z - min) / (max - min) - 1 = a z + b with the codebook's range (train_ldm.py:85-96); {a, b} on the device
            self._range = torch.zeros(2, dtype=F32, device=self.device)
            self.refresh_codebook_range()

    def _models(self):
        return [self.model, self.autoencoder]

    def refresh_codebook_range(self):
        """Re-read min / max of the VQVAE's codebook (one host read: call it after the codebook changed, not inside a step) into the
        device scalars the step and its captured graph read."""
        if self.latent_space_type != "vq":
            raise RuntimeError("refresh_codebook_range() belongs to latent_space_type='vq'")
        self.codebook_min, self.codebook_max = inferer.codebook_range(self.autoencoder)
        self._range.copy_(torch.tensor(inferer.range_forward(self.codebook_min, self.codebook_max), dtype=F32))

    def _latents(self, images, eps):
        """'vae': encode_stage_2_inputs (AEKL:827-830): z = z_mu + eps * z_sigma, fp32 NC[D]HW, unscaled; no tape.
        'vq' (train_ldm.py:54-58): the PRE-quantisation encoder output, no tape, no quantisation; eps must be None."""
        if self.latent_space_type == "vq":
            ae = self.autoencoder
            if eps is not None:
                raise ValueError("eps must be None with latent_space_type='vq': the VQVAE's encoder draws no noise")
            if not images.is_cuda or images.dtype != F32 or not images.is_contiguous():
                raise ValueError("images must be a contiguous fp32 GPU tensor")
            if images.dim() != 5 or images.shape[1] != ae.in_channels:
                raise ValueError(f"images must be NCDHW with {ae.in_channels} channels, got {tuple(images.shape)}")
            ctx = E.Ctx(self.ae_arena, ae._plans, grad_enabled=False, prepacked=ae.pack_all())
            return ops.to_channels_first(ae._run_plan(ctx, ae._enc, ops.to_channels_last(images), False), 3)
        if not (images.is_cuda and eps.is_cuda):  # (this trainer's wording; every other refusal is _encode_sample's)
            raise ValueError("images and eps must be contiguous fp32 GPU tensors")
        z = _encode_sample(self.autoencoder, self.ae_arena, images, eps, False, None, 0.0)[4]
        return ops.to_channels_first(z, self.autoencoder.spatial_dims)

    @torch.no_grad()
    def estimate_scale_factor(self, images, eps):
        """scale_factor = 1 / std(z) over the first batch (T-LDM:110-112); stored and returned ('vae' only)."""
        if self.latent_space_type == "vq":
            raise RuntimeError("latent_space_type='vq' normalises by the codebook's range: there is no scale factor")
        self.scale_factor = float(1.0 / torch.std(self._latents(images, eps)))
        return self.scale_factor

    def _scaled_latents(self, images, eps):
        """latents_scaled = autoencoder.encode_stage_2_inputs(images) * inferer.scale_factor (T-LDM:154-157)."""
        if self.latent_space_type == "vq":  # normalised by the codebook's range instead of a scale factor
            z = self._latents(images, eps)
            call("mi_affine_dev_f32", ptr(z), ptr(self._range), z.numel())
            return z
        if self.scale_factor is None:
            raise RuntimeError("scale_factor is not set: pass it or call estimate_scale_factor(first_batch, eps) (train_ldm.py:110-112)")
        z = self._latents(images, eps)
        call("mi_scale_f32", ptr(z), self.scale_factor, z.numel())
        return z

    def _forward(self, images, eps, noise, timesteps, class_labels=None, context=None, condition=None, drop=None):
        """condition: latent-shaped fp32 tensor (e.g. the label mask resampled to the latent grid) concatenated un-noised behind the
        scaled latents -- BASELINE configs[4]; drop: DDPMTrainer's condition-dropout mask (refused before the encoder runs)."""
        self._check_drop(drop, images, class_labels, context, condition)
        return super()._forward(self._scaled_latents(images, eps), noise, timesteps, class_labels, context, condition, drop)

    def _eval_forward(self, meter, images, eps, noise, timesteps, class_labels=None, context=None, condition=None, drop=None):
        """T-LDM:206-229: latents = autoencoder.encode_stage_2_inputs(images) * scale_factor, then the diffusion batch above."""
        self._check_drop(drop, images, class_labels, context, condition)
        return super()._eval_forward(meter, self._scaled_latents(images, eps), noise, timesteps, class_labels, context, condition, drop)


class AETrainer(_ArenaTrainer):
    """step(images, eps): images fp32 NCDHW, eps fp32 latent-shaped NCDHW (the torch.randn_like of AEKL:786-787 made an
    input so that a captured graph sees fresh noise and tests can pin it).  Defaults are the reference's generator
    optimizer (Adam, lr 5e-5, grad_clip_max_norm 1; T-AE:428-434, 470) and 3-D kl_weight (CFG:995-1026).

    extra_loss: the generator step's third-party terms (T-AE:411-421: `perceptual_loss(recon, images) * perc_weight` and, after the
    warm-up epochs, `adv_loss(discriminator(recon)[-1], target_is_real=True, for_discriminator=False) * adv_weight`).  A callable
    (reconstruction fp32 NCDHW with requires_grad, images) -> scalar torch loss; it runs under torch autograd on the GPU and its
    gradient with respect to the reconstruction joins the L1 gradient before the HIP backward.  The networks inside it
    (`generative`'s PatchDiscriminator / PerceptualLoss with downloaded weights) stay the user's torch modules -- they are not
    rebuilt here.

    perceptual: a perceptual.PerceptualLoss (LPIPS-VGG with the user's weights) run natively inside the step: perc_weight *
    LPIPS(recon, images) joins `loss` (and is kept in the device scalar `perc_loss`), its gradient joins the L1 gradient on the HIP
    path, and capture() / step_graph() include it.  The fake-3D slice indices are drawn on the CPU generator before every step /
    replay (`perc_indices=` pins them).  Both terms may be set; they add.  `reconstruction` (fp32 NCDHW, detached) holds the last step's output for the caller's discriminator step
    (T-AE:371-397), which is plain torch on the caller's side."""

    def __init__(self, model, lr=5e-5, optimizer="Adam", weight_decay=None, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=1.0,
                 kl_weight=1e-7, process_group=None, bucket_mb=64, device=None, grad_accumulate_step=1, extra_loss=None, overlap=None,
                 perceptual=None, perc_weight=0.125, ema_decay=None, ema_warmup=False):
        from .vqvae import VQVAE
        if isinstance(model, VQVAE):
            raise TypeError(f"{type(self).__name__} trains an AutoencoderKL (KL, perceptual and adversarial terms); a VQVAE trains on "
                            "VQAETrainer (L1 + q_weight * quantization loss): perceptual and adversarial terms with a VQVAE are out of scope")
        super().__init__(model, lr, optimizer, weight_decay, betas, eps, max_grad_norm, process_group, bucket_mb, device,
                         grad_accumulate_step, overlap, ema_decay, ema_warmup)
        self.kl_weight = float(kl_weight)
        self.extra_loss = extra_loss
        self.reconstruction = None
        self.extra_loss_value = None
        # native perceptual term (perceptual.PerceptualLoss): perc_weight * LPIPS(recon, images), T-AE:416; the slice indices of a
        # fake-3D loss live in static device buffers refilled before every step / replay (never drawn inside a graph)
        self.perceptual = perceptual
        self.perc_weight = float(perc_weight)
        self.perc_loss = torch.zeros(1, dtype=F32, device=self.device)  # perc_weight * perceptual loss of the last step
        self._perc_idx = None
        if perceptual is not None:
            from .perceptual import PerceptualLoss
            if not isinstance(perceptual, PerceptualLoss):
                raise TypeError("perceptual must be a medical_image_generation_amd.perceptual.PerceptualLoss (torch modules go in extra_loss)")
            perceptual.to(self.device)

    def _fill_perc_indices(self, shape, indices=None):
        """Copy the slice indices of the next step into the static buffers: `indices` (three index tensors) or a fresh draw
        (PerceptualLoss.draw_indices on the CPU generator, as upstream draws in every forward)."""
        if self.perceptual is None:
            return
        if indices is None:
            indices = self.perceptual.draw_indices(tuple(shape))
        if not indices:
            return
        bufs = self._perc_idx
        if bufs is None or [b.numel() for b in bufs] != [i.numel() for i in indices]:
            if self._graph:
                raise ValueError("the slice counts differ from the captured step's")
            bufs = self._perc_idx = [torch.empty(i.numel(), dtype=torch.int32, device=self.device) for i in indices]
        for b, i in zip(bufs, indices):
            b.copy_(i.reshape(-1))

    def step(self, images, eps, last_in_epoch=False, perc_indices=None):
        """perc_indices: the three slice-index tensors of the perceptual term's fake-3D axes (default: a fresh draw)."""
        self._fill_perc_indices(images.shape, perc_indices)
        return super().step(images, eps, last_in_epoch=last_in_epoch)

    def capture(self, images, eps, warmup=2, perc_indices=None):
        self._fill_perc_indices(images.shape, perc_indices)
        super().capture(images, eps, warmup=warmup)
        if self.perceptual is not None:
            self._pinned.append((dict(self.perceptual._plans), self.perceptual._w1, self._perc_idx))

    def step_graph(self, images=None, eps=None, perc_indices=None):
        """Replay; the perceptual term's slice indices are refilled first (fresh draw unless given) -- every replay uses new ones."""
        if self.perceptual is not None and self._graph:
            self._fill_perc_indices(self._static[0].shape, perc_indices)
        return super().step_graph(images, eps)

    def _forward(self, images, eps):
        m = self.model
        ctx, x_cl, mu, sigma, z, (n, lc, lv) = _encode_sample(m, self.arena, images, eps, True, self.loss, self.kl_weight)
        self.arena.grad.zero_()  # (after the inputs were accepted, before anything is written to it: the forward only records)
        tape = ctx.tape

        def bwd():
            dz = tape.take(z)
            dmu, dsigma = torch.empty_like(mu), torch.empty_like(sigma)
            call("mi_reparam_kl_bwd", ptr(mu), ptr(sigma), ptr(eps), ptr(dz), ptr(dmu), ptr(dsigma), n, lc, lv, self.kl_weight)
            tape.put(mu, dmu), tape.put(sigma, dsigma)

        tape.record(bwd)
        recon = m._decode_run(ctx, z, True)
        drecon = torch.empty_like(recon)
        call("mi_l1_fwd_bwd", ptr(recon), ptr(images), ptr(drecon), ptr(self.loss), n, recon.shape[-1], math.prod(images.shape[2:]), 1)
        if self.perceptual is not None:
            self.perc_loss.zero_()
            self.perceptual.hip(recon, x_cl, self._perc_idx, self.perc_loss, self.perc_weight, grad=drecon)  # gradient added into drecon
            ops.add_f32_(self.loss.view(1, 1), self.perc_loss.view(1, 1))
        if self.extra_loss is not None:
            rec = ops.to_channels_first(recon, m.spatial_dims).requires_grad_(True)
            with torch.enable_grad():
                extra = self.extra_loss(rec, images)
                (g,) = torch.autograd.grad(extra, rec)
            self.extra_loss_value = extra.detach()
            self.loss += self.extra_loss_value.to(self.loss.dtype).reshape(self.loss.shape)
            drecon = ops.add(drecon, ops.to_channels_last(g))
            self.reconstruction = rec.detach()
        return tape, recon, drecon

    def _eval_forward(self, meter, images, eps, return_recon=False, kl_meter=None):
        """AutoEncoder.validate_one_epoch's batch (T-AE:447-456): reconstructions, *_ = autoencoder(images) -> l1_loss, and nothing else
        (no KL, perceptual or adversarial term; the discriminator is not run).  AutoencoderKL.forward samples z = mu + eps * sigma in
        eval mode too (AEKL:821-825).  kl_meter: a second ValidationMeter that accounts get_kl_loss(z_mu, z_sigma) of the same batch (the
        loop of adapt_kl_loss_weight, T-AE:295-318).  return_recon: -> the reconstruction as fp32 NC[D]HW (T-AE:463-467: the image pair
        of the epoch's plots)."""
        m = self.model
        if kl_meter is not None and (kl_meter is meter or self._meter(kl_meter) is not kl_meter):
            raise ValueError("kl_meter must be a ValidationMeter of its own")
        ctx, _, mu, sigma, z, (n, lc, lv) = _encode_sample(m, self.arena, images, eps, False, None, 0.0)
        if kl_meter is not None:
            call("mi_kl_eval", ptr(mu), ptr(sigma), ptr(kl_meter.acc), n, lc, lv)
        recon = m._decode_run(ctx, z, False)
        if recon.shape[-1] != images.shape[1] or recon.numel() != images.numel():
            raise ValueError(f"the reconstruction has shape {tuple(recon.shape)} (channels-last) for images {tuple(images.shape)}")
        call("mi_l1_eval", ptr(recon), ptr(images), ptr(meter.acc), n, recon.shape[-1], math.prod(images.shape[2:]))
        return ops.to_channels_first(recon, m.spatial_dims) if return_recon else None


class AEGANTrainer(AETrainer):
    """The autoencoder's GAN step with BOTH networks on the HIP path (train_autoencoder.AutoEncoder.train_one_epoch, T-AE:371-435):

        generator      (T-AE:406-435): recon = AE(images); loss_g = L1 + kl_weight * KL [+ extra_loss] + (adversarial: after the warm-up
                       epochs, T-AE:416) adv_weight * LS(D(recon)[-1], real)  ->  backward through D (frozen) and the AE -> clip -> Adam
        discriminator  (T-AE:371-397): loss_d = adv_weight * 0.5 * (LS(D(recon.detach())[-1], fake) + LS(D(images)[-1], real))
                       ->  backward through D -> clip -> Adam (lr 5e-5, T-AE:471)

    `discriminator`: medical_image_generation_amd.discriminator.PatchDiscriminator; LS = PatchAdversarialLoss("least_squares").
    step(images, eps) runs both (the reference's order: generator, then discriminator on the same reconstruction); `adversarial`
    switches the adversarial term and the discriminator step on (epoch >= autoencoder_warm_up_epochs).  The perceptual term is
    AETrainer's `perceptual=` (native) or the caller's `extra_loss`.  capture() / step_graph() replay generator and discriminator graphs."""

    def __init__(self, model, discriminator, adv_weight=0.01, d_lr=5e-5, adversarial=True, **kw):
        super().__init__(model, **kw)
        if self.grad_accumulate_step != 1:
            raise NotImplementedError("AEGANTrainer covers grad_accumulate_step == 1")
        from .discriminator import PatchAdversarialLoss
        self.D = discriminator
        self.d_arena = discriminator.arena(self.device)
        if self.world > 1:
            ddp.broadcast_parameters(self.d_arena.data, 0, self.pg)
        self.adv, self.adv_weight = PatchAdversarialLoss("least_squares"), float(adv_weight)
        self.adversarial = bool(adversarial)
        n = self.d_arena.n_trainable
        self.d_exp_avg = torch.zeros(n, dtype=F32, device=self.device)
        self.d_exp_avg_sq = torch.zeros(n, dtype=F32, device=self.device)
        self.d_step_count = torch.zeros(1, dtype=F32, device=self.device)
        # torch.optim.Adam(discriminator.parameters(), lr=d_lr) (T-AE:471): the generator's betas / eps / clip norm, no weight decay;
        # no averaged weights either: only the autoencoder is sampled from
        self.d_optimizer = FusedAdam(discriminator, self.d_arena, self.d_exp_avg, self.d_exp_avg_sq, self.d_step_count, d_lr, self.betas,
                                     self.eps, 0.0, False, self.max_grad_norm, 1.0 / self.world)
        self.d_sumsq = self.d_optimizer.sumsq
        self.gen_loss = torch.zeros(1, dtype=F32, device=self.device)   # adv_weight * LS(D(recon), real) of the last generator step
        self.disc_loss = torch.zeros(1, dtype=F32, device=self.device)  # adv_weight * 0.5 (fake + real) of the last discriminator step
        self.recon_cl = None
        self._g_d = None

    d_lr = property(lambda self: self.d_optimizer.lr, lambda self, v: setattr(self.d_optimizer, "lr", v))

    @property
    def max_grad_norm(self):
        return self.optimizer.max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, v):  # one clip norm for both networks (T-AE:393, 431)
        self.optimizer.max_grad_norm = v
        if hasattr(self, "d_optimizer"):
            self.d_optimizer.max_grad_norm = v

    def _forward(self, images, eps):
        tape, recon, drecon = super()._forward(images, eps)
        self.recon_cl = recon
        if self.adversarial:
            self.gen_loss.zero_()
            c = E.Ctx(self.d_arena, {}, grad_enabled=True)
            logits = self.D._run(c, recon, need_dx=True, param_grads=False)[-1]  # D frozen: `requires_grad = False` (T-AE:401-402)
            dl = self.adv.hip(logits, True, self.gen_loss, self.adv_weight)
            c.tape.backward(logits, dl)
            g = c.tape.take(recon)
            c.tape.grads.clear(), c.tape.keep.clear()
            drecon = ops.add(drecon, g)
            ops.add_f32_(self.loss.view(1, 1), self.gen_loss.view(1, 1))
        return tape, recon, drecon

    # ---- discriminator step
    def d_forward_backward(self, images):
        """Gradients of loss_d into d_arena.grad (fresh), loss into self.disc_loss; uses the reconstruction of the last generator step."""
        if self.recon_cl is None:
            raise RuntimeError("run the generator step first (the discriminator step scores ITS reconstruction, T-AE:376)")
        self.d_arena.grad.zero_()
        self.disc_loss.zero_()
        for x_cl, real in ((self.recon_cl, False), (ops.to_channels_last(images), True)):
            c = E.Ctx(self.d_arena, {}, grad_enabled=True)
            logits = self.D._run(c, x_cl, need_dx=False)[-1]
            dl = self.adv.hip(logits, real, self.disc_loss, 0.5 * self.adv_weight)
            c.tape.backward(logits, dl)
            c.tape.grads.clear(), c.tape.keep.clear()

    def _d_exchange(self):
        if self.world > 1:
            a = self.d_arena
            ddp.GradientExchange(a.grad, 0, a.n_trainable, self.pg, self.bucket_elems).finish()

    def d_optimizer_step(self):
        self._d_exchange()
        self.d_optimizer.step()

    def step(self, images, eps, last_in_epoch=False, perc_indices=None):
        loss = super().step(images, eps, perc_indices=perc_indices)
        if self.adversarial:
            self.d_forward_backward(images)
            self.d_optimizer_step()
        return loss

    def capture(self, images, eps, warmup=2, perc_indices=None):
        """The warm-up passes run the discriminator in training mode on whatever the graph pool holds; its BatchNorm running buffers
        are restored afterwards, so capture() leaves them (and checkpoints of them) exactly as they were."""
        bn = [b.clone() for b in self.D.buffers()]
        try:
            self._capture(images, eps, warmup, perc_indices)
        finally:
            torch.cuda.synchronize()
            for b, s in zip(self.D.buffers(), bn):
                b.copy_(s)

    def _capture(self, images, eps, warmup, perc_indices):
        super().capture(images, eps, warmup=warmup, perc_indices=perc_indices)
        if self.adversarial:
            self._warm_up(lambda: self.d_forward_backward(self._static[0]), 1)
            self.d_optimizer.push()
            self._d_clip_captured = self.d_optimizer.clip
            self._g_d = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._g_d, pool=self._g_fb.pool(), capture_error_mode="thread_local"):
                self.d_forward_backward(self._static[0])
                if self.world <= 1:
                    self.d_optimizer.launch()
            self._pinned.append((self.d_arena, dict(ops._ws_cache)))

    def step_graph(self, images=None, eps=None, perc_indices=None):
        loss = super().step_graph(images, eps, perc_indices=perc_indices)
        if self._g_d is not None:
            self._check_clip(self.d_optimizer, self._d_clip_captured)
            if self.world > 1:
                self._g_d.replay()
                self.d_optimizer_step()
            else:
                self.d_optimizer.step(replay=self._g_d)  # discriminator forward / backward + its optimizer, block refreshed first
        return loss


class VQAETrainer(_ArenaTrainer):
    """The autoencoder's train step under `--latent_space_type vq` (train_autoencoder.py:407-414 with `generative`'s VQVAE):

        recon, quantization_loss = VQVAE(images);  loss = L1(recon, images) + q_weight * quantization_loss  ->  backward -> clip -> Adam

    step(images): images fp32 NCDHW.  The nearest-code search, the straight-through gather, the commitment loss and the EMA codebook
    update (training mode, after the gather) run inside the step and inside its captured graph (csrc/vq.hip; no host synchronisation,
    bit-reproducible; the L1 loss, the clip norm and the bias gradients of this step are fixed-order reductions too, so a captured step
    equals the eager one bit for bit).  `q_weight` lives in a device scalar, so a captured graph follows a changed weight.  The codebook and its EMA
    buffers are not in the arena: neither the optimizer nor the clip norm sees them.  `q_loss` holds the last step's quantization loss
    (unweighted), `vqvae.quantizer.perplexity` the codebook usage.  validate() runs the eval-mode forward (no codebook update) and
    accounts the L1 term, as AETrainer does (T-AE:447-456).  Perceptual and adversarial terms are out of scope."""

    def __init__(self, model, q_weight=1.0, lr=5e-5, optimizer="Adam", weight_decay=None, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=1.0,
                 process_group=None, bucket_mb=64, device=None, grad_accumulate_step=1, overlap=None, ema_decay=None, ema_warmup=False):
        from .vqvae import VQVAE
        if not isinstance(model, VQVAE):
            raise TypeError("VQAETrainer trains a medical_image_generation_amd.vqvae.VQVAE (an AutoencoderKL trains on AETrainer)")
        world = dist.get_world_size(process_group) if (process_group is not None or dist.is_initialized()) else 1
        if world > 1 and model.ddp_sync:
            raise NotImplementedError("ddp_sync=True over a process group of size > 1: the all-reduce of the codebook counts and sums is "
                                      "not on the HIP path")
        super().__init__(model, lr, optimizer, weight_decay, betas, eps, max_grad_norm, process_group, bucket_mb, device,
                         grad_accumulate_step, overlap, ema_decay, ema_warmup)
        self._q_weight = torch.full((1,), float(q_weight), dtype=F32, device=self.device)
        self.q_loss = torch.zeros(1, dtype=F32, device=self.device)
        # fixed-order loss and clip-norm reductions: the captured step is bit-equal to the eager one
        self._partials = torch.empty(constants()["MI_VQ_PARTIALS"], dtype=torch.float64, device=self.device)
        self.optimizer.fixed_order_norm()

    def capture(self, images, warmup=2):
        """The warm-up passes run the step's kernels, the EMA codebook update among them, without an optimizer step: the quantiser
        tensors and the perplexity are put back afterwards, so capture() leaves state_dict() as it found it."""
        q = self.model.quantizer
        live = (q.quantizer.embedding.weight.data, q.quantizer.ema_cluster_size, q.quantizer.ema_w, q.perplexity)
        saved = [t.clone() for t in live]
        try:
            super().capture(images, warmup=warmup)
        finally:
            torch.cuda.synchronize()
            for t, s0 in zip(live, saved):
                t.copy_(s0)

    @property
    def q_weight(self) -> float:
        return float(self._q_weight)

    @q_weight.setter
    def q_weight(self, v):
        self._q_weight.fill_(float(v))

    def _check(self, images):
        m = self.model
        if not images.is_cuda:
            raise RuntimeError("VQAETrainer inputs must live on the GPU")
        if images.dtype != F32 or not images.is_contiguous():
            raise ValueError("images must be a contiguous fp32 GPU tensor")
        if images.dim() != 5 or images.shape[1] != m.in_channels:
            raise ValueError(f"images must be NCDHW with {m.in_channels} channels, got {tuple(images.shape)}")

    def _run(self, images, grad_enabled, update):
        m = self.model
        self._check(images)
        x_cl = ops.to_channels_last(images)
        ctx = E.Ctx(self.arena, m._plans, grad_enabled=grad_enabled, prepacked=m.pack_all())
        z = m._run_plan(ctx, m._enc, x_cl, False)
        zq, diff, _, _ = m._quantize_cl(z, update=update, loss=self.q_loss if grad_enabled else None)
        if ctx.tape is not None:
            from .vqvae import vq_bwd
            tape = ctx.tape
            scale = 2.0 * m.commitment_cost / z.numel()

            def bwd():  # straight-through: dz = dq + q_weight * 2 cc (z - q) / numel
                dq = tape.take(zq)
                tape.put(z, vq_bwd(dq, diff, self._q_weight, scale))

            tape.record(bwd)
        recon = m._run_plan(ctx, m._dec, zq, True)
        if recon.shape[-1] != images.shape[1] or recon.numel() != images.numel():
            raise ValueError(f"the reconstruction has shape {tuple(recon.shape)} (channels-last) for images {tuple(images.shape)}")
        return ctx, recon

    def _forward(self, images):
        ctx, recon = self._run(images, True, self.model.training)
        self.arena.grad.zero_()  # (the forward only records)
        drecon = torch.empty_like(recon)
        call("mi_l1_fwd_bwd_det", ptr(recon), ptr(images), ptr(drecon), ptr(self.loss), ptr(self._partials), recon.shape[0], recon.shape[-1],
             math.prod(images.shape[2:]))
        call("mi_axpy_dev_f32", ptr(self.loss), ptr(self.q_loss), ptr(self._q_weight), 1)
        return ctx.tape, recon, drecon

    def _eval_forward(self, meter, images, return_recon=False):
        _, recon = self._run(images, False, False)
        call("mi_l1_eval", ptr(recon), ptr(images), ptr(meter.acc), recon.shape[0], recon.shape[-1], math.prod(images.shape[2:]))
        return ops.to_channels_first(recon, 3) if return_recon else None
