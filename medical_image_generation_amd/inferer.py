"""Reverse-diffusion sampling on the HIP path: the loop behind `inferer.sample(...)` in LDM.sample_images (train_ldm.py:332-366) and
DDPM.sample_image (train_ddpm.py:238-246).

The reference takes `DDPMScheduler`, `DiffusionInferer` and `LatentDiffusionInferer` from the third-party `generative` package
(train_ldm.py:74, 102, 112), which is not under /root/reference; the classes here mirror the part of their interface those call
sites use (same names, argument meaning, return values).  The scheduler arithmetic is the closed form of Ho et al. 2020 as upstream
implements it, restated in oracle/step.py (`DDPMSchedule.step`): PARITY UNPINNED -- the reference holds no vectors for it; the
tests pin the kernel against that restatement.

One denoising step = UNet forward (no tape) + ONE fused update launch (`mi_diffusion_step`: predicted x0, clip, the scheduler's update,
noise; it also writes the next step's channels-last bf16 model input), captured once as a hipGraph and replayed per timestep -- the
timestep is a device scalar the embedding and update kernels read, so all 1000 steps share one graph.  Every loop below makes that
one call, with NULL for what it was not built with (guidance scale, known region).

Few-step sampling and image-to-noise inversion go through `DDIMScheduler` (third-party `generative` as well, Song et al. 2021 as
upstream implements it, restated in tests/ddim_ref.py: PARITY UNPINNED): the same loop and launch with `ddim` set, which reads row i
of a per-run table of step constants, so step count, eta and direction change without a new capture.  The scheduler kind reaches the
loop in that argument alone; the rest it asks of the `_Scheduler` interface.

Class-conditional models sample with `class_labels=`.  Classifier-free guidance (`guidance_scale=`; Ho & Salimans 2022 -- not part of the
reference; PARITY UNPINNED): every step is ONE forward at batch 2N -- the conditional half [0, N) and the null half [N, 2N) -- and the
update launch forms m = m_uncond + w (m_cond - m_uncond) and continues with the unguided arithmetic.  Null means zeros for the
cross-attention context and the concatenated condition channels, and `null_class` for the class route -- what
trainer.DDPMTrainer(..., null_class=).step(..., drop) trains.  w is a device scalar: one graph serves every scale.

Image-conditioned sampling (`img2img`, `inpaint`; SDEdit, Meng et al. 2022, and masked inpainting in the manner of RePaint, Lugmayr et al.
2022 -- not part of the reference; PARITY UNPINNED): a run may start part-way down the step list, from the image noised to that level,
and with a mask every step is still ONE forward plus ONE launch, which composites inside the update: the generated value where the
mask is 1, the known image at the level the step arrives at where it is 0 (a per-step `known` table beside the step table).
Resampling is a list of moves: denoising steps, replayed from the same graph, and forward-diffusion moves (`mi_renoise`) between them.
Mask, image and known-region noise are buffers, the known rows a table the captured step already points at; the start and the move list
only choose which replays happen: one captured graph serves every run-time choice.

Tiled sampling (`window_inferer=` on sample / img2img / invert; MultiDiffusion, Bar-Tal et al. 2023 -- not part of the reference; PARITY
UNPINNED; off unless called): a whole case from a patch-trained U-Net.  At every step the model runs on overlapping windows of its
training extent, the window predictions are blended, and the scheduler's update is applied to the whole case.  Given the sample x fp32
[N, C, *S], an optional concat condition cond [N, Cc, *S], the windows o_k and extent roi of sliding.WindowPlan(S, roi_size, overlap),
the importance map imp (fp32, built as SlidingWindowInferer builds it), the model f and a step at timestep t:

    p_k      = f(cat(x[n, :, o_k : o_k+roi], cond[n, :, o_k : o_k+roi]), t, context_n, label_n)   # bf16 NDHWC model output, read as fp32
    guided:    p_k = p_k(null condition) + w * (p_k(condition) - p_k(null condition))             # per window, before the blend, fp32
    acc[n,c,v] = sum_k imp[v-o_k] * p_k[c, v-o_k]
    wsum[v]    = sum_k imp[v-o_k]
    m[n,c,v]   = acc[n,c,v] / wsum[v]                                                             # IEEE division
    x[n,c,v]  <- ddpm_update / ddim_update(x, m, z, row of this step)

Each term of acc is one fused multiply-add, in flat window order n * num_windows + w, as `mi_sw_accumulate` does it; wsum sums in the
same order.  The update is the plain step's own arithmetic (the same device functions, flags, table row and device scalar index), so one
window that covers the case in mode="constant" is the plain sampler bit for bit.  There is no padding: a case smaller than roi on any axis
is a ValueError, because a noise sample has no border to mirror.  wsum does not change during a run and is computed once per run.
Filler rows of the last window batch run the model on zeros and are never accumulated.  Class labels and context rows belong to each
window's image n and are staged per window batch like the table rows.  The voxel passes are `mi_sw_gather_cl` (the model input of a
window batch straight from x and cond), `mi_sw_accumulate_cl` (blend, guided combination first) and `mi_sw_diffusion_step` (division,
update, acc = 0) in csrc/sliding.hip; one captured gather -> U-Net -> accumulate body is replayed per window batch (`_TiledLoop`), so
eager and captured runs are bit-equal and nothing synchronises with the host inside a run.  `inpaint` is not tiled.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import engine as E
from . import hipops as ops
from ._lib import call, ptr

F32 = torch.float32


def betas(schedule, num_train_timesteps, beta_start, beta_end):
    """The fp32 betas of generative's schedulers, for training (trainer.DDPMSchedule) and sampling (DDPMScheduler) alike."""
    if schedule == "scaled_linear_beta":
        return torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=F32) ** 2
    if schedule == "linear_beta":
        return torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=F32)
    raise ValueError(f"unknown schedule {schedule}")


def _known_rows(a, a_next):
    """fp32 [len(a), 4] = sqrt(A_next), sqrt(1 - A_next), sqrt(A_t / A_next), sqrt(1 - A_t / A_next) for steps that leave the level a
    (fp64) and arrive at a_next: the known region at the arrival level is [0] image + [1] noise (`mi_diffusion_step`), and [2] x + [3] noise
    takes a sample back from a_next to a (`mi_renoise`).  fp64 with every radicand clamped at 0, kept as fp32."""
    q = a / a_next
    return torch.stack([a_next.clamp(min=0).sqrt(), (1 - a_next).clamp(min=0).sqrt(), q.clamp(min=0).sqrt(), (1 - q).clamp(min=0).sqrt()],
                       dim=1).float().contiguous()


def resample_moves(n_steps, jump_length, jump_n_sample, start=0):
    """The move list of a resampled ("time travel") run over steps start .. n_steps - 1: [("d", i) | ("n", i), ...] -- ("d", i) is
    denoising step i, ("n", i) undoes step i with one forward-diffusion move (`mi_renoise`).  The d moves run in order; each time the
    number of completed steps p (counted from `start`) reaches a multiple of jump_length with steps left, jump_n_sample - 1 times:
    n for the last jump_length steps, newest first, then d for the same steps again.  Jumps never go above `start`.
        resample_moves(4, 2, 2) = d0 d1 n1 n0 d0 d1 d2 d3;   forwards: n + (r - 1) j floor((n - 1) / j) for n = n_steps - start
    In the manner of RePaint (Lugmayr et al. 2022), but the order is this project's own: PARITY UNPINNED."""
    n, j, r = int(n_steps) - int(start), int(jump_length), int(jump_n_sample)
    if start < 0 or n < 1:
        raise ValueError(f"resample: start {start} leaves no step of {n_steps}")
    if j < 1 or r < 1 or j > n:
        raise ValueError(f"resample: jump_length must lie in [1, {n}] and jump_n_sample be at least 1, got ({jump_length}, {jump_n_sample})")
    moves = []
    for i in range(start, n_steps):
        moves.append(("d", i))
        if (i + 1 - start) % j == 0 and i + 1 < n_steps:
            for _ in range(r - 1):
                moves += [("n", k) for k in range(i, i - j, -1)]
                moves += [("d", k) for k in range(i - j + 1, i + 1)]
    return moves


class _Scheduler:
    """What both schedulers share: the beta schedule, the checks, add_noise / get_velocity, the per-device tables, and what the fused
    loop asks of either -- `ddim`, `flags`, [known_]coefficients(), known_rows(), _steps, _fill, _index, _draws (the defaults: DDPM's)."""
    ddim = 0  # the table form the update kernel reads: 0 = [T][5] coefficients indexed by t, 1 = per-run rows indexed by the step

    def __init__(self, num_train_timesteps, schedule, clip_sample, prediction_type, beta_start, beta_end):
        if prediction_type not in ("epsilon", "v_prediction"):
            raise ValueError(f"unknown prediction_type {prediction_type}")
        self.betas = betas(schedule, num_train_timesteps, beta_start, beta_end)
        self.num_train_timesteps, self.prediction_type, self.clip_sample = num_train_timesteps, prediction_type, clip_sample
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self._dev = {}

    @property
    def flags(self):  # of the update kernel: bit 0 = clip_sample, bit 1 = v-prediction
        return int(self.clip_sample) | (2 if self.prediction_type == "v_prediction" else 0)

    def _stride(self, num_inference_steps):
        if num_inference_steps > self.num_train_timesteps:
            raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than `self.num_train_timesteps`: "
                             f"{self.num_train_timesteps}")
        return self.num_train_timesteps // num_inference_steps

    def _device_table(self, name, device, make):
        """A device table, allocated once per device (make() -> its host form): a captured graph that points at it stays valid."""
        table = self._dev.get(name)
        if table is None or table.device != torch.device(device):
            table = self._dev[name] = make().to(device)
        return table

    def _levels(self, like, timesteps):
        a = self.alphas_cumprod.to(like.device)[timesteps]
        shape = (-1,) + (1,) * (like.ndim - 1)
        return (a ** 0.5).reshape(shape), ((1 - a) ** 0.5).reshape(shape)

    def add_noise(self, original_samples, noise, timesteps):
        sa, sb = self._levels(original_samples, timesteps)
        return sa * original_samples + sb * noise

    def get_velocity(self, sample, noise, timesteps):
        sa, sb = self._levels(sample, timesteps)
        return sa * noise - sb * sample

    def _steps(self, reverse=False):  # the timesteps in the order the loop takes them
        return [int(t) for t in (self.timesteps.flip(0) if reverse else self.timesteps)]

    def _fill(self, coef, known, known_rows, index, eta, reverse):
        """This run's rows into the device tables the (possibly captured) step reads; DDPM's hold every timestep: nothing to do."""

    def _index(self, i, t):  # what the update kernel indexes its tables with at step i, timestep t
        return t

    def _draws(self, t, eta, reverse):  # whether the step at timestep t reads z (sigma != 0)
        return t > 0


class DDPMScheduler(_Scheduler):
    """`generative.networks.schedulers.DDPMScheduler` as train_ldm.py:74 constructs it (variance_type "fixed_small")."""

    def __init__(self, num_train_timesteps=1000, schedule="linear_beta", variance_type="fixed_small", clip_sample=True,
                 prediction_type="epsilon", beta_start=1e-4, beta_end=2e-2):
        if variance_type != "fixed_small":
            raise NotImplementedError("only variance_type='fixed_small' (the upstream default the reference uses)")
        super().__init__(num_train_timesteps, schedule, clip_sample, prediction_type, beta_start, beta_end)
        acp, b = self.alphas_cumprod.double(), self.betas.double()
        prev = torch.cat([torch.ones(1, dtype=torch.float64), acp[:-1]])
        sigma = ((1 - prev) / (1 - acp) * b).clamp(min=1e-20).sqrt()
        sigma[0] = 0.0  # no noise is added at t = 0
        self._coef = torch.stack([1 / acp.sqrt(), (1 - acp).sqrt(), prev.sqrt() * b / (1 - acp), (1 - b).sqrt() * (1 - prev) / (1 - acp), sigma],
                                 dim=1).float().contiguous()
        self.set_timesteps(num_train_timesteps)

    def set_timesteps(self, num_inference_steps, device=None):
        ratio = self._stride(num_inference_steps)
        self.num_inference_steps = num_inference_steps
        timesteps = (torch.arange(0, num_inference_steps) * ratio).round().flip(0).to(torch.int64)
        self.timesteps = timesteps if device is None else timesteps.to(device)

    def coefficients(self, device):
        return self._device_table("coef", device, lambda: self._coef)

    def known_rows(self):
        """fp32 [T, 4], row t: the known-region constants (`_known_rows`) of the step that leaves t -- it arrives at alphas_cumprod[t - 1]
        (1 at t = 0), the level this scheduler's coefficients assume whatever the stride."""
        acp = self.alphas_cumprod.double()
        return _known_rows(acp, torch.cat([torch.ones(1, dtype=torch.float64), acp[:-1]]))

    def known_coefficients(self, device):
        """The device table `mi_diffusion_step` reads beside coefficients(): [num_train_timesteps, 4]."""
        return self._device_table("known", device, self.known_rows)

    def step(self, model_output, timestep, sample, generator=None):
        """(pred_prev_sample, pred_original_sample) for fp32 NC[D]HW tensors -- the upstream signature; the fused loop of the inferers
        below does not go through this (tensor-level) method."""
        t = int(timestep)
        k = self._coef[t].to(sample.device)
        if self.prediction_type == "v_prediction":
            x0 = sample / k[0] - k[1] * model_output
        else:
            x0 = (sample - k[1] * model_output) * k[0]
        if self.clip_sample:
            x0 = x0.clamp(-1, 1)
        prev = k[2] * x0 + k[3] * sample
        if t > 0:
            prev = prev + k[4] * torch.randn(sample.shape, generator=generator, device=sample.device, dtype=sample.dtype)
        return prev, x0


class DDIMScheduler(_Scheduler):
    """`generative.networks.schedulers.DDIMScheduler`: the few-step sampler that passes to the same `inferer.sample(..., scheduler=...)`
    call (train_ldm.py:351-364), and `reversed_step`, image-to-noise inversion.  The upstream source is absent; the arithmetic is the
    closed form of Song et al. 2021 as upstream implements it, restated in tests/ddim_ref.py: PARITY UNPINNED -- the reference holds
    no vectors for it.

    Unlike a strided DDPMScheduler, whose coefficients take alphas_cumprod[t-1] as the previous level whatever the stride, the
    previous level here is alphas_cumprod[t - T // n]: this is the scheduler to use with n < T steps.

    Per-step constants are rows [r0..r4] = sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev-sigma^2), sigma, built in fp64 with
    every radicand clamped at 0 and kept as fp32; the update for sample x, model output m, noise z:
        epsilon: x0 = (x - r1 m) / r0, e = m;    v_prediction: x0 = r0 x - r1 m, e = r0 m + r1 x
        x_next = r2 clip(x0) + r3 e + r4 z       (e is not recomputed from the clipped x0)"""
    ddim = 1

    def __init__(self, num_train_timesteps=1000, schedule="linear_beta", clip_sample=True, set_alpha_to_one=True, steps_offset=0,
                 prediction_type="epsilon", beta_start=1e-4, beta_end=2e-2):
        super().__init__(num_train_timesteps, schedule, clip_sample, prediction_type, beta_start, beta_end)
        self.steps_offset = steps_offset
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]  # the level "before" t = 0
        self.first_alpha_cumprod = torch.tensor(0.0)  # the level "after" t = T - 1 (inversion): pure noise
        # every training timestep, descending; steps_offset shifts the strided subsets of set_timesteps only
        self.num_inference_steps = num_train_timesteps
        self.timesteps = torch.arange(num_train_timesteps - 1, -1, -1, dtype=torch.int64)

    def set_timesteps(self, num_inference_steps, device=None):
        ratio = self._stride(num_inference_steps)
        timesteps = (torch.arange(0, num_inference_steps) * ratio).flip(0).to(torch.int64) + self.steps_offset
        if int(timesteps[0]) >= self.num_train_timesteps:
            raise ValueError(f"`steps_offset`: {self.steps_offset} moves the largest of {num_inference_steps} timesteps to "
                             f"{int(timesteps[0])}, past `self.num_train_timesteps`: {self.num_train_timesteps}")
        self.num_inference_steps = num_inference_steps
        self.timesteps = timesteps if device is None else timesteps.to(device)

    def _rows(self, t, eta=0.0, reverse=False):
        """fp32 [len(t), 5]: the constants of the steps that leave the timesteps t (int64), towards t - ratio (denoising) or
        t + ratio (reverse=True), computed in fp64."""
        acp, ratio = self.alphas_cumprod.double(), self.num_train_timesteps // self.num_inference_steps
        t = t.cpu()
        a = acp[t]
        if reverse:
            p = t + ratio
            ap = torch.where(p < self.num_train_timesteps, acp[p.clamp(max=self.num_train_timesteps - 1)], self.first_alpha_cumprod.double())
            sigma = torch.zeros_like(a)
        else:
            p = t - ratio
            ap = torch.where(p >= 0, acp[p.clamp(min=0)], self.final_alpha_cumprod.double())
            sigma = eta * ((1 - ap) / (1 - a) * (1 - a / ap)).clamp(min=0).sqrt()
        return torch.stack([a.sqrt(), (1 - a).clamp(min=0).sqrt(), ap.sqrt(), (1 - ap - sigma ** 2).clamp(min=0).sqrt(), sigma], dim=1).float()

    def rows(self, eta=0.0, reverse=False):
        """One row per step in the order the loop takes them: self.timesteps, or ascending for reverse=True (inversion)."""
        return self._rows(self.timesteps.flip(0) if reverse else self.timesteps, eta, reverse).contiguous()

    def coefficients(self, device):
        """[num_train_timesteps, 5]: full capacity, valid over set_timesteps, eta and direction -- the loop refills it (`_fill`)."""
        return self._device_table("coef", device, lambda: torch.zeros(self.num_train_timesteps, 5, dtype=F32))

    def known_rows(self, eta=0.0):
        """fp32 [n_steps, 4] in loop order: the known-region constants (`_known_rows`) of the denoising steps, each arriving at the `ap` of
        its row (final_alpha_cumprod on the last).  eta does not enter: the marginal at the next level is ap whatever sigma is."""
        acp, ratio = self.alphas_cumprod.double(), self.num_train_timesteps // self.num_inference_steps
        t = self.timesteps.cpu()
        p = t - ratio
        return _known_rows(acp[t], torch.where(p >= 0, acp[p.clamp(min=0)], self.final_alpha_cumprod.double()))

    def known_coefficients(self, device):
        """The device table `mi_diffusion_step` reads beside coefficients(): [num_train_timesteps, 4], refilled like it."""
        return self._device_table("known", device, lambda: torch.zeros(self.num_train_timesteps, 4, dtype=F32))

    def _fill(self, coef, known, known_rows, index, eta, reverse):
        rows = self.rows(eta, reverse)
        coef[:len(rows)].copy_(rows)
        index.zero_()  # the warm-up and capture passes read row 0
        if known is not None:
            known[:len(known_rows)].copy_(known_rows)

    def _index(self, i, t):
        return i

    def _draws(self, t, eta, reverse):
        return not (reverse or eta == 0)  # deterministic rows (sigma = 0): the kernel does not read z

    def _update(self, r, model_output, sample):
        if self.prediction_type == "v_prediction":
            x0, e = r[0] * sample - r[1] * model_output, r[0] * model_output + r[1] * sample
        else:
            x0, e = (sample - r[1] * model_output) / r[0], model_output
        if self.clip_sample:
            x0 = x0.clamp(-1, 1)
        return r[2] * x0 + r[3] * e, x0

    def step(self, model_output, timestep, sample, eta=0.0, generator=None):
        """(prev_sample, pred_original_sample) for fp32 NC[D]HW tensors -- the upstream signature; plain torch on any device (the
        fused loop of the inferers below does not go through the tensor-level methods)."""
        r = self._rows(torch.tensor([int(timestep)]), eta)[0].to(sample.device)
        prev, x0 = self._update(r, model_output, sample)
        if eta > 0:
            prev = prev + r[4] * torch.randn(sample.shape, generator=generator, device=sample.device, dtype=sample.dtype)
        return prev, x0

    def reversed_step(self, model_output, timestep, sample):
        """(post_sample, pred_original_sample): one deterministic step towards noise, from `timestep` to `timestep + ratio`."""
        r = self._rows(torch.tensor([int(timestep)]), reverse=True)[0].to(sample.device)
        return self._update(r, model_output, sample)


class _Noise:
    """Where the noise of one run comes from.  z, one per move: noises[j], else drawn from `generator`.  zk, the noise of an inpaint
    loop's known region: known_noises -- one tensor, or one per "d" move --, else drawn: before every "d" move (fresh), or once, before
    the first pass.  The loop asks per "d" move for z, then zk: the order of the draws."""

    def __init__(self, noises=None, generator=None, known_noises=None, fresh=False):
        self.noises, self.generator, self.known_noises = noises, generator, known_noises
        self.per_move = fresh if known_noises is None else not torch.is_tensor(known_noises)  # zk changes with every "d" move

    def _put(self, buf, pinned):
        if pinned is not None:
            buf.copy_(pinned)
        else:
            buf.normal_(generator=self.generator)

    def z(self, buf, j):
        self._put(buf, None if self.noises is None else self.noises[j])

    def zk(self, buf, done=None):
        """done None: before the first pass, where a once-per-run zk is set; else before "d" move number `done`."""
        if self.per_move == (done is not None):
            self._put(buf, self.known_noises[done] if self.per_move and self.known_noises is not None else self.known_noises)


class _Loop:
    """One captured denoising step, replayed over scheduler.timesteps."""

    def __init__(self, model, scheduler, shape, device, cond_channels=0, context_shape=None, guided=False, labels=False, inpaint=False):
        """cond_channels: channels of a mode="concat" conditioning tensor that sit, un-noised, behind the sample's channels in the model
        input; context_shape: (tokens, cross_attention_dim) of a mode="crossattn" conditioning; labels: the model reads class labels;
        guided: classifier-free guidance -- the model runs at batch 2N (condition, then null condition), the sample stays at batch N;
        inpaint: the update launch composites with this loop's image, mask [N, V], known-region noise and known table."""
        self.m, self.sch = model, scheduler
        n, c = shape[0], shape[1]
        self.guided = bool(guided)
        sp = tuple(shape[2:])
        self.v = math.prod(sp)
        self.n, self.c = n, c
        self.x = torch.empty(shape, dtype=F32, device=device)                    # the sample, fp32 NC[D]HW
        self.cc = int(cond_channels)
        self._model_buffers(n, sp, device, context_shape, labels)
        self.w = torch.ones(1, dtype=F32, device=device) if self.guided else None  # the guidance scale the guided update kernel reads
        self.z = torch.empty(shape, dtype=F32, device=device)
        self.t = torch.zeros(1, dtype=torch.int64, device=device)   # what the update kernel indexes its tables with (scheduler._index)
        self.coef = scheduler.coefficients(device)
        self.inpaint = bool(inpaint)
        self.image = self.mask = self.zk = self.known = None
        if self.inpaint:
            self.image = torch.zeros(shape, dtype=F32, device=device)       # the known content, at the sample's level of abstraction
            self.mask = torch.ones((n, self.v), dtype=F32, device=device)   # 1: regenerate, 0: keep, between: blend
            self.zk = torch.zeros(shape, dtype=F32, device=device)          # the noise of the known region
            self.known = scheduler.known_coefficients(device)
        self.arena = model.arena(device)
        self.graph = None
        self.keys = ()  # conv plans whose weights are packed: once per run(), not per step (the weights do not change while sampling)
        self._pinned = None  # objects whose device memory the captured graph points at (conv plans, GroupNorm workspace)
        self.captures = 0

    def _model_buffers(self, rows, sp, device, context_shape, labels):
        """What the model reads: `rows` samples of spatial extent `sp` (twice as many when guided)."""
        nb = 2 * rows if self.guided else rows  # the model's batch
        dims = (1,) * (3 - len(sp)) + tuple(sp)
        self.x_cl = torch.empty((nb,) + dims + (self.c + self.cc,), dtype=torch.bfloat16, device=device)  # the sample as the model reads it (+ condition)
        self.ctx = None if context_shape is None else torch.empty((nb * context_shape[0], context_shape[1]), dtype=torch.bfloat16, device=device)
        self.labels = torch.zeros(nb, dtype=torch.int64, device=device) if labels else None
        self.tn = torch.zeros(nb, dtype=torch.int64, device=device)  # the timestep the model reads

    def _body(self):  # what is captured
        self._step()

    def _advance(self):  # one denoising move
        if self.graph is not None:
            self.graph.replay()
        else:
            self._step()

    def _step(self):
        ctx = E.Ctx(self.arena, self.m._plans, grad_enabled=False, prepacked=self.keys)
        eps = self.m._run(ctx, self.x_cl, self.tn, need_dx=False, class_labels=self.labels, context=self.ctx)
        # NULL for what the loop was not built with: w (unguided: eps and x_cl of batch N), the known region (the plain step)
        call("mi_diffusion_step", ptr(self.x), ptr(eps), ptr(self.z), ptr(self.coef), ptr(self.t), ptr(self.w), ptr(self.mask), ptr(self.image),
             ptr(self.zk), ptr(self.known), ptr(self.x_cl), self.c + self.cc, self.n, self.c, self.v, self.sch.flags, self.sch.ddim)

    def _load(self, x):
        """x (fp32 NC[D]HW) -> the sample channels of the model input (the condition channels behind them stay)."""
        self.x.copy_(x)
        x_cl = ops.to_channels_last(self.x)
        for h in range(2 if self.guided else 1):
            self.x_cl[h * self.n:(h + 1) * self.n, ..., :self.c].copy_(x_cl)

    def _load_condition(self, conditioning, class_labels, guidance_scale, null_class):
        """What the loop was built for (concat channels or context, labels, guided), filled before any step."""
        n = self.n
        if self.cc:  # mode="concat": model_input = cat([image, conditioning], dim=1) at every step; written once, the steps rewrite `image`
            self.x_cl[:n, ..., self.c:].copy_(ops.to_channels_last(conditioning))
        elif self.ctx is not None:  # mode="crossattn": the context token matrix is a constant of the loop
            self.ctx[:n * conditioning.shape[1]].copy_(ops.cast_bf16(conditioning.contiguous().reshape(-1, conditioning.shape[2])))
        if self.labels is not None:
            self.labels[:n].copy_(class_labels)
        if self.guided:  # the null half: zero condition channels, zero context tokens, the null class
            if self.cc:
                self.x_cl[n:, ..., self.c:].zero_()
            elif self.ctx is not None:
                self.ctx[n * conditioning.shape[1]:].zero_()
            if self.labels is not None:
                self.labels[n:].fill_(null_class)
            self.w.fill_(float(guidance_scale))

    def _load_known(self, image, mask, noise):  # the known region: its content, the mask ([N or 1, 1, *spatial]), a once-per-run zk
        self.image.copy_(image)
        self.mask.copy_(mask.to(device=self.x.device, dtype=F32).expand((self.n,) + tuple(mask.shape[1:])).reshape(self.n, -1))
        noise.zk(self.zk)

    def run(self, x, noise, cond, known=None, use_graph=True, on_step=None, eta=0.0, reverse=False, start=0, moves=None):
        """x: the sample of step `start` (an index into the step list); noise: a `_Noise`; cond: `_load_condition`'s arguments; known:
        (image, mask as `inpaint` takes it), an inpaint loop's known content.
        eta, reverse: DDIM only -- the noise scale of the denoising rows; reverse=True runs the inversion rows over ascending timesteps.
        moves: the list `resample_moves` returns, default one "d" per step from `start` -- noise.noises holds one z per move."""
        if self.m._arena is not self.arena:  # the module moved (.to / .cuda): plans and graph point at the old buffers -> start over
            self.arena, self.graph, self.keys, self._pinned = self.m.arena(self.x.device), None, (), None
        if reverse and (self.inpaint or start or moves is not None):
            raise ValueError("the inversion rows take no mask, start or move list")
        self._load_condition(*cond)
        self._load(x)
        steps = self.sch._steps(reverse)
        if moves is None:
            moves = [("d", i) for i in range(start, len(steps))]
        # the host's copy of the known rows: mi_renoise takes its two factors by value
        rows = self.sch.known_rows() if self.inpaint or any(kind == "n" for kind, _ in moves) else None
        self.sch._fill(self.coef, self.known, rows, self.t, eta, reverse)  # the tables of THIS run, before any step runs
        if self.inpaint:
            self._load_known(*known, noise)
        keep = self.x.clone()
        if not self.m._plans or len(self.keys) != len(self.m._plans):
            self.keys = ()
            self.z.zero_()
            self._body()  # first pass at this shape: creates the conv plans, every conv packs its own weights
        self.keys = self.m.pack_all()  # current weights, one launch
        if use_graph and self.graph is None and len(steps) > 2:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self.z.zero_()
                self._body()  # workspaces (hipMalloc) outside the capture
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
                self._body()
            self.captures += 1
            self._pinned = (dict(self.m._plans), dict(ops._ws_cache), self.arena)  # keep what the graph points at alive
        self._load(keep)
        self._walk(moves, steps, rows, noise, eta, reverse, on_step)
        return self.x.clone()

    def _walk(self, moves, steps, rows, noise, eta, reverse, on_step):
        done = 0  # "d" moves so far
        for j, (kind, i) in enumerate(moves):
            t = steps[i]
            if kind == "n":  # undo step i: one forward-diffusion move from the level it arrived at, eager, between two replays
                noise.z(self.z, j)
                row = rows[self.sch._index(i, t)]
                call("mi_renoise", ptr(self.x), ptr(self.z), float(row[2]), float(row[3]), ptr(self.x_cl), self.c + self.cc, self.n,
                     2 if self.guided else 1, self.c, self.v)
                continue
            self.t.fill_(self.sch._index(i, t))
            self.tn.fill_(t)
            if self.sch._draws(t, eta, reverse):
                noise.z(self.z, j)
            if self.inpaint:
                noise.zk(self.zk, done)
            done += 1
            self._advance()
            if on_step is not None:
                on_step(i, t, self.x)


class _TiledLoop(_Loop):
    """The loop of a whole case under a patch-trained model (module docstring, "Tiled sampling"): x, z, acc and wsum have the case's
    extent, the model's buffers that of one window batch.  One captured gather -> U-Net -> accumulate body is replayed per window
    batch after that batch's table rows, labels and context were copied (device to device) into the buffers it reads; the update
    launch follows the last batch."""

    def __init__(self, model, scheduler, shape, device, window, cond_channels=0, context_shape=None, guided=False, labels=False):
        from . import sliding  # here, not at the top: the trainers import this module and tile nothing
        sp = tuple(int(s) for s in shape[2:])
        plan = window.plan(sp)
        if plan.padded != sp:
            raise ValueError(f"window_inferer: the case {sp} is smaller than the window {plan.roi}: a noise sample has no border to pad")
        self.plan, self.b = plan, window.sw_batch_size
        self.roi3 = sliding._dims3(plan.roi)
        self.tokens = None if context_shape is None else int(context_shape[0])
        super().__init__(model, scheduler, shape, device, cond_channels, context_shape, guided, labels)
        n = self.n
        self.imp = window._importance(plan.roi, torch.device(device))(plan.roi)
        self.acc = torch.zeros(shape, dtype=F32, device=device)
        self.wsum = torch.zeros(sp, dtype=F32, device=device)
        self.cond = torch.empty((n, self.cc) + sp, dtype=F32, device=device) if self.cc else None  # the concat condition of the whole case
        # the window table of every batch (row 0: N, D, H, W of the case), staged once; `table` is the one the kernels read
        rows = sliding._rows3(plan.rows(n, self.b), len(sp))
        self.calls = rows.shape[0]
        head = np.asarray([n] + list(sliding._dims3(sp)), np.int32)
        host = np.concatenate([np.broadcast_to(head, (self.calls, 1, 4)), rows], axis=1)
        self.host_tables = torch.from_numpy(np.ascontiguousarray(host))
        self.tables = self.host_tables.to(device)
        self.table = self.tables[0].clone()
        # the image every row belongs to (fillers: image 0, masked out): labels and context rows are staged per batch with it
        image = torch.from_numpy(rows[..., 0].astype(np.int64))
        self.row_valid = (image >= 0).to(device)
        self.row_image = image.clamp(min=0).to(device)
        self.labels_all = self.ctx_all = None

    def _model_buffers(self, rows, sp, device, context_shape, labels):
        super()._model_buffers(self.b, self.plan.roi, device, context_shape, labels)

    def _load(self, x):
        self.x.copy_(x)
        self.acc.zero_()  # the passes that created plans and workspaces accumulated into it

    def _load_condition(self, conditioning, class_labels, guidance_scale, null_class):
        """The whole-case condition, the labels and context rows of every window batch (each row's image's own; fillers and the null
        half: zeros / `null_class`), the guidance scale, and the weight sum, which does not change during a run."""
        calls, b = self.calls, self.b
        nb = 2 * b if self.guided else b
        if self.cc:
            self.cond.copy_(conditioning)
        elif self.ctx is not None:
            tokens = ops.cast_bf16(conditioning.contiguous().reshape(-1, conditioning.shape[2])).reshape(self.n, self.tokens, -1)
            self.ctx_all = torch.zeros((calls, nb, self.tokens, tokens.shape[2]), dtype=torch.bfloat16, device=self.x.device)
            self.ctx_all[:, :b] = tokens[self.row_image] * self.row_valid[..., None, None]
            self.ctx_all = self.ctx_all.reshape(calls, nb * self.tokens, -1)
        if self.labels is not None:
            self.labels_all = torch.zeros((calls, nb), dtype=torch.int64, device=self.x.device)
            self.labels_all[:, :b] = class_labels[self.row_image] * self.row_valid
            if self.guided:
                self.labels_all[:, b:] = int(null_class)
        if self.guided:
            self.w.fill_(float(guidance_scale))
        self.wsum.zero_()
        for k in range(calls):
            call("mi_sw_accumulate_cl", None, None, ptr(self.imp), ptr(self.tables[k]), self.host_tables[k].data_ptr(), b, self.c, *self.roi3,
                 ptr(self.acc), ptr(self.wsum), self.acc.numel())
        self._stage(0)  # the passes before the first step run on the first batch

    def _stage(self, k):
        self.table.copy_(self.tables[k])
        if self.labels is not None:
            self.labels.copy_(self.labels_all[k])
        if self.ctx is not None:
            self.ctx.copy_(self.ctx_all[k])

    def _body(self):
        """gather -> U-Net -> accumulate on the batch the static table names; no host table: the kernels guard themselves."""
        call("mi_sw_gather_cl", ptr(self.x), self.x.numel(), self.c, ptr(self.cond), self.cond.numel() if self.cc else 0, self.cc, ptr(self.table),
             None, self.b, int(self.guided), *self.roi3, ptr(self.x_cl))
        ctx = E.Ctx(self.arena, self.m._plans, grad_enabled=False, prepacked=self.keys)
        eps = self.m._run(ctx, self.x_cl, self.tn, need_dx=False, class_labels=self.labels, context=self.ctx)
        if tuple(eps.shape) != tuple(self.x_cl.shape[:-1]) + (self.c,):
            raise ValueError(f"the model returned {tuple(eps.shape)} for windows of {tuple(self.x_cl.shape)}: its output must have the "
                             f"sample's {self.c} channels and the window's extent")
        call("mi_sw_accumulate_cl", ptr(eps), ptr(self.w), ptr(self.imp), ptr(self.table), None, self.b, self.c, *self.roi3, ptr(self.acc), None,
             self.acc.numel())

    def _step(self):
        for k in range(self.calls):
            self._stage(k)
            if self.graph is not None:
                self.graph.replay()
            else:
                self._body()
        call("mi_sw_diffusion_step", ptr(self.x), ptr(self.acc), ptr(self.wsum), ptr(self.z), ptr(self.coef), ptr(self.t), self.n, self.c, self.v,
             self.sch.flags, self.sch.ddim)

    def _advance(self):
        self._step()


class DiffusionInferer:
    """`generative.inferers.DiffusionInferer(scheduler)`: `sample(input_noise, diffusion_model, scheduler)` (train_ddpm.py:243)."""

    def __init__(self, scheduler):
        self.scheduler = scheduler
        self._loops = {}

    def _loop(self, model, scheduler, shape, device, cond_channels=0, context_shape=None, guided=False, labels=False, inpaint=False,
              window=None):
        """window: a `sliding.SlidingWindowInferer` -> the tiled loop of a case of this shape under its windows."""
        tiling = None
        if window is not None:
            per_axis = lambda v: tuple(v) if isinstance(v, (tuple, list)) else v  # noqa: E731
            tiling = (per_axis(window.roi_size), window.sw_batch_size, per_axis(window.overlap), window.mode, per_axis(window.sigma_scale))
        key = (id(model), id(scheduler), tuple(shape), cond_channels, context_shape, bool(guided), bool(labels), bool(inpaint), tiling)
        if key not in self._loops:
            if window is None:
                self._loops[key] = _Loop(model, scheduler, tuple(shape), device, cond_channels, context_shape, guided, labels, inpaint)
            else:
                self._loops[key] = _TiledLoop(model, scheduler, tuple(shape), device, window, cond_channels, context_shape, guided, labels)
        return self._loops[key]

    @staticmethod
    def _check_mode(mode):
        if mode not in ("crossattn", "concat"):
            raise NotImplementedError(f"{mode} condition is not supported")

    def __call__(self, inputs, diffusion_model, noise, timesteps, condition=None, mode="crossattn"):
        """The training-side call of train_ddpm.py:191: `noise_pred = inferer(inputs=images, diffusion_model=model, noise=noise,
        timesteps=timesteps)` = diffusion_model(scheduler.add_noise(inputs, noise, timesteps), timesteps) (third-party
        `generative.inferers.DiffusionInferer.__call__`).  Differentiable through the model's autograd edge; the fused
        trainer.DDPMTrainer is the fast path for the same computation."""
        self._check_mode(mode)
        noisy = self.scheduler.add_noise(original_samples=inputs, noise=noise, timesteps=timesteps)
        if mode == "concat" and condition is not None:  # un-noised condition channels behind the noised ones; no cross-attention context
            noisy, condition = torch.cat([noisy, condition.to(noisy.dtype)], dim=1), None
        return diffusion_model(x=noisy, timesteps=timesteps, context=condition)

    def _conditioning(self, x, diffusion_model, conditioning, mode, class_labels=None, guidance_scale=None, null_class=None):
        """The checks of a sample / invert call -> (conditioning as fp32 on x's device, concat channels, cross-attention context shape,
        class labels as int64 [N] on x's device or None)."""
        self._check_mode(mode)
        if not x.is_cuda:
            raise RuntimeError("medical_image_generation_amd runs on MI355X only: move the inputs to 'cuda'")
        cc, ctx_shape = 0, None
        if conditioning is not None:
            conditioning = conditioning.to(device=x.device, dtype=F32).contiguous()
            if mode == "concat":
                if conditioning.dim() != x.dim() or conditioning.shape[0] != x.shape[0] or conditioning.shape[2:] != x.shape[2:]:
                    raise ValueError("mode='concat': conditioning must have the sample's batch and spatial shape")
                cc = conditioning.shape[1]
            else:
                if not getattr(diffusion_model, "with_conditioning", False):
                    raise ValueError("model should have with_conditioning = True if context is provided")
                if conditioning.dim() != 3 or conditioning.shape[0] != x.shape[0] or \
                        conditioning.shape[2] != diffusion_model.cross_attention_dim:
                    raise ValueError(f"mode='crossattn': conditioning must be [batch, tokens, {diffusion_model.cross_attention_dim}]")
                ctx_shape = (conditioning.shape[1], conditioning.shape[2])
        elif getattr(diffusion_model, "with_conditioning", False):
            raise ValueError("the model was built with_conditioning=True: pass conditioning=[batch, tokens, cross_attention_dim]")
        if x.shape[1] + cc != diffusion_model.in_channels:
            raise ValueError(f"Input number of channels ({x.shape[1] + cc}) is not equal to expected number of channels "
                             f"({diffusion_model.in_channels})")
        nce = getattr(diffusion_model, "num_class_embeds", None)
        if (class_labels is None) != (nce is None):
            raise ValueError("class_labels should be provided exactly when the model has num_class_embeds")
        if class_labels is not None:  # the kernels index the embedding table with them: nn.Embedding's range check, on the host
            class_labels = torch.as_tensor(class_labels).to(device=x.device, dtype=torch.int64).contiguous()
            if class_labels.shape != (x.shape[0],) or int(class_labels.min()) < 0 or int(class_labels.max()) >= nce:
                raise ValueError(f"class_labels must hold one index in [0, {nce}) per sample")
        if guidance_scale is not None:
            if conditioning is None and class_labels is None:
                raise ValueError("guidance_scale: there is no conditioning to guide with (no conditioning=, no class_labels=)")
            if class_labels is not None and (null_class is None or not 0 <= int(null_class) < nce):
                raise ValueError(f"guidance on a class-conditional model needs null_class= in [0, {nce}): the label of the unconditional branch")
        return conditioning, cc, ctx_shape, class_labels

    def _run(self, image, diffusion_model, scheduler, conditioning, mode, class_labels, guidance_scale, null_class, noise, input_noise=None,
             start=0, mask=None, window_inferer=None, **how):
        """The one path from the arguments of sample / img2img / inpaint / invert to the loop and its run.  image: the run's shape and, at
        start > 0 or under a (checked) mask, its content; noise: a `_Noise`; window_inferer: None, or the windows of the tiled loop; how:
        what `_Loop.run` takes besides."""
        if window_inferer is not None and mask is not None:
            raise NotImplementedError("window_inferer= is not supported by inpaint: the tiled loop has no known region")
        conditioning, cc, ctx_shape, class_labels = self._conditioning(image, diffusion_model, conditioning, mode, class_labels,
                                                                       guidance_scale, null_class)
        x = self._first_sample(image, input_noise, scheduler, start, noise.generator)
        known = None if mask is None else (image.float(), mask)
        loop = self._loop(diffusion_model, scheduler, image.shape, image.device, cc, ctx_shape, guidance_scale is not None,
                          class_labels is not None, mask is not None, window_inferer)
        return loop.run(x, noise, (conditioning, class_labels, guidance_scale, null_class), known, start=start, **how)

    @torch.no_grad()
    def sample(self, input_noise, diffusion_model, scheduler=None, save_intermediates=False, intermediate_steps=100, conditioning=None,
               mode="crossattn", verbose=True, noises=None, generator=None, use_graph=True, eta=0.0, class_labels=None,
               guidance_scale=None, null_class=None, window_inferer=None):
        """conditioning with mode="concat": fp32 NC'[D]HW, model_input = cat([image, conditioning], dim=1) at every step; with
        mode="crossattn": fp32 [N, tokens, cross_attention_dim], the model's `context` (train_ldm.py:349-365 passes neither).
        noises: optional sequence with the z of every step (tests pin them); generator: torch generator for the per-step noise.
        eta: the noise scale of a DDIMScheduler (0 = deterministic; no per-step noise is drawn); other schedulers ignore it.
        class_labels: int64 [N], for a model built with num_class_embeds.
        guidance_scale: a float w selects classifier-free guidance (not part of the reference; PARITY UNPINNED): the model output of
        every step is m_uncond + w (m_cond - m_uncond), from one forward at batch 2N whose second half carries the null condition --
        zero context tokens, zero condition channels, and `null_class` (required with class_labels) as the label.  w = 1 is the
        conditional model, w = 0 the unconditional one; the scale is a device scalar, so all scales share one captured graph.
        window_inferer: a `sliding.SlidingWindowInferer` selects tiled sampling (module docstring; not part of the reference; PARITY
        UNPINNED) for a case larger than the model's training patch: its roi_size, sw_batch_size, overlap, mode and sigma_scale are
        used (its padding settings are not: a case smaller than the roi on any axis is a ValueError).  None: the plain loop."""
        inter = []

        def on_step(i, t, x):
            if save_intermediates and t % intermediate_steps == 0:
                inter.append(x.clone())

        image = self._run(input_noise, diffusion_model, scheduler or self.scheduler, conditioning, mode, class_labels, guidance_scale, null_class,
                          _Noise(noises, generator), input_noise, window_inferer=window_inferer, use_graph=use_graph, on_step=on_step, eta=eta)
        return (image, inter) if save_intermediates else image

    @staticmethod
    def _start(scheduler, strength):
        """strength in (0, 1] -> the index into scheduler.timesteps of the first step taken: the last min(int(n strength), n) steps run."""
        n = len(scheduler.timesteps)
        n_run = min(int(n * strength), n) if 0 < strength <= 1 else 0
        if n_run == 0:
            raise ValueError(f"strength must lie in (0, 1] and leave at least one of the {n} steps, got {strength}")
        return n - n_run

    @staticmethod
    def _first_sample(image, input_noise, scheduler, start, generator):
        """The sample a run enters step `start` with: input_noise itself at start 0, else the image noised to that step's level."""
        if input_noise is None:
            input_noise = torch.randn(image.shape, generator=generator, device=image.device, dtype=F32)
        if tuple(input_noise.shape) != tuple(image.shape):
            raise ValueError("input_noise must have the image's shape")
        if start == 0:
            return input_noise.float()
        return scheduler.add_noise(image.float(), input_noise.float(), int(scheduler.timesteps[start]))

    @staticmethod
    def _check_mask(mask, shape):
        if not torch.is_tensor(mask) or not (mask.dtype == torch.bool or mask.is_floating_point()):
            raise ValueError("mask must be a bool or float tensor (1: regenerate, 0: keep)")
        if mask.dim() != len(shape) or mask.shape[1] != 1 or mask.shape[0] not in (1, shape[0]) or tuple(mask.shape[2:]) != tuple(shape[2:]):
            raise ValueError(f"mask must be [N, 1, *spatial] or [1, 1, *spatial] for an image of shape {tuple(shape)}, got {tuple(mask.shape)}")

    @staticmethod
    def _refuse_mask(mask):
        if mask is not None:
            raise ValueError("invert takes no mask: the inversion rows have no known region (use inpaint to regenerate one)")

    @torch.no_grad()
    def img2img(self, image, diffusion_model, strength, input_noise=None, scheduler=None, conditioning=None, mode="crossattn", verbose=True,
                noises=None, generator=None, use_graph=True, eta=0.0, class_labels=None, guidance_scale=None, null_class=None,
                window_inferer=None):
        """Partial-noise start (SDEdit's `strength`; the noise-and-reconstruct recipe of anomaly maps; not part of the reference: PARITY
        UNPINNED): the last n_run = min(int(n strength), n) of the scheduler's n steps, from scheduler.add_noise(image, input_noise,
        timesteps[n - n_run]) -- or from input_noise itself when all n run: strength 1 is `sample(input_noise)`.  The loop, kernels and
        captured graph of `sample`; the other arguments as there (`noises`: one z per step taken)."""
        scheduler = scheduler or self.scheduler
        start = self._start(scheduler, strength)
        return self._run(image, diffusion_model, scheduler, conditioning, mode, class_labels, guidance_scale, null_class,
                         _Noise(noises, generator), input_noise, start, window_inferer=window_inferer, use_graph=use_graph, eta=eta)

    @torch.no_grad()
    def inpaint(self, image, mask, diffusion_model, strength=1.0, input_noise=None, known_noise=None, known_noises=None, resample=None,
                scheduler=None, conditioning=None, mode="crossattn", verbose=True, noises=None, generator=None, use_graph=True, eta=0.0,
                class_labels=None, guidance_scale=None, null_class=None, on_step=None, window_inferer=None):
        """Regenerate the region where mask is 1 so that it agrees with the image kept where mask is 0 (in the manner of RePaint, Lugmayr
        et al. 2022; not part of the reference: PARITY UNPINNED).  mask: bool or float [N, 1, *spatial] or [1, 1, *spatial]; values
        between 0 and 1 blend (a feathered edge).  After every step the kept region is the image at the level the step arrived at,
        sqrt(A_next) image + sqrt(1 - A_next) zk, written by the step's own update launch; with set_alpha_to_one (or DDPM's t = 0) the
        last level is the image itself, so kept voxels come back exactly.
        strength, input_noise: as `img2img` (strength 1 starts from input_noise).
        known_noise: "fixed" -- zk is drawn once per run (deterministic with DDIM eta = 0) -- or "fresh" -- redrawn before every
        denoising move, as RePaint does; None: "fresh" when the sampler draws per-step noise (DDPM, DDIM with eta > 0), else "fixed".
        known_noises pins zk: one tensor, or one per denoising move.
        resample=(jump_length, jump_n_sample): `resample_moves` -- without it the region does not harmonise with its surroundings when
        the model was not trained for inpainting.  noises: one z per move of either kind, in move order.
        on_step(i, t, x): called after every denoising move.  The other arguments as `sample`, except window_inferer: tiled sampling
        has no known region (NotImplementedError)."""
        scheduler = scheduler or self.scheduler
        self._check_mask(mask, image.shape)
        start = self._start(scheduler, strength)
        if known_noise not in (None, "fixed", "fresh"):
            raise ValueError(f"known_noise must be 'fixed', 'fresh' or None, got {known_noise!r}")
        moves = None if resample is None else resample_moves(len(scheduler.timesteps), resample[0], resample[1], start)
        fresh = (not isinstance(scheduler, DDIMScheduler) or eta > 0) if known_noise is None else known_noise == "fresh"
        return self._run(image, diffusion_model, scheduler, conditioning, mode, class_labels, guidance_scale, null_class,
                         _Noise(noises, generator, known_noises, fresh), input_noise, start, mask, window_inferer, use_graph=use_graph,
                         on_step=on_step, eta=eta, moves=moves)

    @torch.no_grad()
    def invert(self, image, diffusion_model, scheduler=None, conditioning=None, mode="crossattn", use_graph=True, class_labels=None,
               guidance_scale=None, null_class=None, mask=None, window_inferer=None):
        """Image-to-noise DDIM inversion: DDIMScheduler.reversed_step over ascending timesteps in the fused loop of `sample` (same
        captured graph, the reverse rows in its table).  Returns the noise-side sample, fp32.  PARITY UNPINNED, as the scheduler.
        class_labels, guidance_scale, null_class, window_inferer: as in `sample`.  mask: refused -- there is no inversion of a masked
        region."""
        self._refuse_mask(mask)
        scheduler = scheduler or self.scheduler
        if not isinstance(scheduler, DDIMScheduler):
            raise TypeError(f"invert needs a DDIMScheduler (reversed_step), not {type(scheduler).__name__}")
        return self._run(image, diffusion_model, scheduler, conditioning, mode, class_labels, guidance_scale, null_class, _Noise(), image,
                         window_inferer=window_inferer, use_graph=use_graph, reverse=True)


class LatentDiffusionInferer(DiffusionInferer):
    """`generative.inferers.LatentDiffusionInferer(scheduler, scale_factor)`: samples latents, then decodes
    `autoencoder_model.decode_stage_2_outputs(latents / scale_factor)` (train_ldm.py:112, 362-364).

    `decode_inferer=` on sample / img2img / inpaint (not part of upstream): a `sliding.SlidingWindowInferer` whose roi_size is in
    latent voxels; the final decode then runs window by window (`sliding.tiled_decode`), for latents larger than the patch the
    autoencoder was trained on.  None: the plain decode.

    `window_inferer=` on sample / img2img / invert: tiled sampling of the latent (DiffusionInferer.sample), its roi_size in latent
    voxels too; with `decode_inferer=` a patch-trained pair produces a whole case end to end.  The encoding inside img2img / invert
    is not tiled."""

    def __init__(self, scheduler, scale_factor=1.0):
        super().__init__(scheduler)
        self.scale_factor = scale_factor

    def _decode(self, autoencoder_model, latent, decode_inferer=None):
        if decode_inferer is None:
            return autoencoder_model.decode_stage_2_outputs(latent / self.scale_factor)
        from .sliding import tiled_decode  # here, not at the top: the trainers import this module and tile nothing
        return tiled_decode(autoencoder_model, latent / self.scale_factor, decode_inferer)

    def __call__(self, inputs, autoencoder_model, diffusion_model, noise, timesteps, condition=None, mode="crossattn"):
        """`generative.inferers.LatentDiffusionInferer.__call__`: encode (no grad) -> * scale_factor -> DiffusionInferer.__call__."""
        with torch.no_grad():
            latent = autoencoder_model.encode_stage_2_inputs(inputs) * self.scale_factor
        return super().__call__(inputs=latent, diffusion_model=diffusion_model, noise=noise, timesteps=timesteps, condition=condition,
                                mode=mode)

    @torch.no_grad()
    def sample(self, input_noise, autoencoder_model, diffusion_model, scheduler=None, save_intermediates=False, intermediate_steps=100,
               conditioning=None, mode="crossattn", verbose=True, noises=None, generator=None, use_graph=True, eta=0.0, class_labels=None,
               guidance_scale=None, null_class=None, decode_inferer=None, window_inferer=None):
        out = super().sample(input_noise, diffusion_model, scheduler, save_intermediates, intermediate_steps, conditioning, mode, verbose,
                             noises=noises, generator=generator, use_graph=use_graph, eta=eta, class_labels=class_labels,
                             guidance_scale=guidance_scale, null_class=null_class, window_inferer=window_inferer)
        latent, inter = out if save_intermediates else (out, None)
        image = self._decode(autoencoder_model, latent, decode_inferer)
        if save_intermediates:
            return image, [self._decode(autoencoder_model, z, decode_inferer) for z in inter]
        return image

    @torch.no_grad()
    def invert(self, image, autoencoder_model, diffusion_model, scheduler=None, conditioning=None, mode="crossattn", use_graph=True,
               class_labels=None, guidance_scale=None, null_class=None, mask=None, window_inferer=None):
        """DDIM inversion of the latent: DiffusionInferer.invert(encode_stage_2_inputs(image) * scale_factor); the encoding is the
        plain one also when the inversion is tiled (`window_inferer=`)."""
        self._refuse_mask(mask)
        latent = autoencoder_model.encode_stage_2_inputs(image) * self.scale_factor
        return super().invert(latent, diffusion_model, scheduler, conditioning, mode, use_graph, class_labels, guidance_scale, null_class,
                              window_inferer=window_inferer)

    @torch.no_grad()
    def img2img(self, image, autoencoder_model, diffusion_model, strength, input_noise=None, decode_inferer=None, **kwargs):
        """DiffusionInferer.img2img on encode_stage_2_inputs(image) * scale_factor (input_noise has the latent's shape), then decoded."""
        latent = autoencoder_model.encode_stage_2_inputs(image) * self.scale_factor
        latent = super().img2img(latent, diffusion_model, strength, input_noise, **kwargs)
        return self._decode(autoencoder_model, latent, decode_inferer)

    @staticmethod
    def latent_mask(mask, latent_spatial):
        """An image-space mask [N, 1, *spatial] on the latent grid: the mean over each latent voxel's footprint (a box of image extent /
        latent extent per axis, which must be an integer) -- a soft mask, fp32, fractional where the footprint straddles the edge."""
        sp = tuple(mask.shape[2:])
        if len(sp) != len(latent_spatial) or any(l < 1 or s % l for s, l in zip(sp, latent_spatial)):
            raise ValueError(f"mask extent {sp} is no integer multiple of the latent extent {tuple(latent_spatial)}")
        f = tuple(s // l for s, l in zip(sp, latent_spatial))
        pool = {1: torch.nn.functional.avg_pool1d, 2: torch.nn.functional.avg_pool2d, 3: torch.nn.functional.avg_pool3d}[len(sp)]
        return pool(mask.float(), kernel_size=f, stride=f)

    @torch.no_grad()
    def inpaint(self, image, mask, autoencoder_model, diffusion_model, strength=1.0, input_noise=None, paste_back=True, decode_inferer=None,
                **kwargs):
        """DiffusionInferer.inpaint in the latent space: the image encoded (* scale_factor), the mask reduced by `latent_mask` (once per
        call), the loop, then decoded.  paste_back: return mask * decoded + (1 - mask) * image in image space -- the autoencoder is
        lossy, and known voxels must come back exactly.  input_noise and the pinned noises have the latent's shape."""
        self._check_mask(mask, image.shape)
        latent = autoencoder_model.encode_stage_2_inputs(image) * self.scale_factor
        out = super().inpaint(latent, self.latent_mask(mask, latent.shape[2:]), diffusion_model, strength, input_noise, **kwargs)
        out = self._decode(autoencoder_model, out, decode_inferer)
        if paste_back:
            m = mask.to(device=out.device, dtype=out.dtype)
            out = m * out + (1 - m) * image.to(out.dtype)
        return out


# ------------------------------------------------------------------------------------------------ VQ latents (train_ldm.py -l vq)
def codebook_range(autoencoder):
    """(min, max) of a VQVAE's codebook as Python floats: ONE host read (train_ldm.py:85-96 reads them once per run)."""
    cb = autoencoder.codebook.data
    return float(cb.min()), float(cb.max())


def range_forward(lo, hi):
    """{a, b} of x0 = 2 (z - lo) / (hi - lo) - 1 = a z + b."""
    return 2.0 / (hi - lo), -2.0 * lo / (hi - lo) - 1.0


def range_inverse(lo, hi):
    """{a, b} of z = (x0 + 1) / 2 * (hi - lo) + lo = a x0 + b."""
    return (hi - lo) / 2.0, (hi + lo) / 2.0


class VQLatentDiffusionInferer(DiffusionInferer):
    """The inferer of train_ldm.py's `vq` branch (:68-69, 85-105, 149-152, 355-360): the diffusion model works on the VQVAE's
    PRE-quantisation encoder output normalised to [-1, 1] by the codebook's min / max; a sample is renormalised, quantised and decoded.
    The range is read once (`refresh_codebook_range()` re-reads it) and kept as device scalars; both affine maps are one
    `mi_affine_dev_f32` launch.  `normalize` / `denormalize` are public so that a caller can compose the pieces by hand."""

    def __init__(self, scheduler, autoencoder):
        from .vqvae import VQVAE
        if not isinstance(autoencoder, VQVAE):
            raise TypeError("VQLatentDiffusionInferer takes a medical_image_generation_amd.vqvae.VQVAE (an AutoencoderKL: LatentDiffusionInferer)")
        super().__init__(scheduler)
        self.autoencoder = autoencoder
        self._fwd = self._inv = None
        self.refresh_codebook_range()

    def refresh_codebook_range(self):
        self.codebook_min, self.codebook_max = codebook_range(self.autoencoder)
        dev = self.autoencoder.codebook.device
        self._fwd = torch.tensor(range_forward(self.codebook_min, self.codebook_max), dtype=F32, device=dev)
        self._inv = torch.tensor(range_inverse(self.codebook_min, self.codebook_max), dtype=F32, device=dev)

    def _affine(self, x, ab):
        if not x.is_cuda:
            raise RuntimeError("medical_image_generation_amd runs on MI355X only (no CPU fallback)")
        y = x.detach().to(F32).clone(memory_format=torch.contiguous_format)
        call("mi_affine_dev_f32", ptr(y), ptr(ab.to(y.device)), y.numel())
        return y

    def normalize(self, z):
        """2 (z - min) / (max - min) - 1 (no gradient: the encoder is frozen in the LDM loop)."""
        return self._affine(z, self._fwd)

    def denormalize(self, x):
        """(x + 1) / 2 * (max - min) + min."""
        return self._affine(x, self._inv)

    def decode(self, latent):
        """Renormalise, quantise (no codebook update, whatever the module's mode) and decode (train_ldm.py:355-360)."""
        ae = self.autoencoder
        z_cl = ops.to_channels_last(self.denormalize(latent))
        zq = ae._quantize_cl(z_cl, update=False)[0]
        return ae.decode(ops.to_channels_first(zq, 3))

    def __call__(self, inputs, diffusion_model, noise, timesteps, condition=None, mode="crossattn"):
        with torch.no_grad():
            latent = self.normalize(self.autoencoder.encode_stage_2_inputs(inputs))
        return super().__call__(inputs=latent, diffusion_model=diffusion_model, noise=noise, timesteps=timesteps, condition=condition,
                                mode=mode)

    @torch.no_grad()
    def sample(self, input_noise, diffusion_model, scheduler=None, save_intermediates=False, intermediate_steps=100, conditioning=None,
               mode="crossattn", verbose=True, noises=None, generator=None, use_graph=True, eta=0.0, class_labels=None,
               guidance_scale=None, null_class=None, decode_inferer=None, window_inferer=None):
        """DiffusionInferer.sample on the latent shape (the same captured loop; DDIM, guidance and class_labels pass through), then
        `decode`.  Windowed sampling and windowed decoding are not built for VQ latents."""
        if window_inferer is not None or decode_inferer is not None:
            raise NotImplementedError("window_inferer / decode_inferer: windowed sampling and decoding are not built for VQ latents")
        out = super().sample(input_noise, diffusion_model, scheduler, save_intermediates, intermediate_steps, conditioning, mode, verbose,
                             noises=noises, generator=generator, use_graph=use_graph, eta=eta, class_labels=class_labels,
                             guidance_scale=guidance_scale, null_class=null_class)
        if save_intermediates:
            return self.decode(out[0]), [self.decode(z) for z in out[1]]
        return self.decode(out)
