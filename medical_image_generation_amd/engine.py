"""Tape engine: forward ops on channels-last bf16 activations that record their own HIP backward.

Why not one torch.autograd.Function per kernel: the fused kernels need to know about each other
(a conv's epilogue emits the channel sums the NEXT GroupNorm's statistics come from; the conv's data gradient
feeds the GroupNorm/SiLU backward which also folds in the other gradient branches of the same tensor), and
gradient accumulation must run through our kernels, not aten::add.  The tape gives that control; `functional.py` wraps whole
blocks / networks of it as torch.autograd.Function for callers that want autograd.

Everything here launches HIP kernels through hipops; torch only allocates (torch.empty / views).
"""
from __future__ import annotations

import math
import weakref

import torch

from . import _lib
from . import hipops as ops
from ._lib import call, ptr

BF16, F32 = torch.bfloat16, torch.float32

import os as _os
# Backward schedules that were measured and not kept (second-stream or deferred weight gradients, data gradient first, the two-launch
# GroupNorm backward, GroupNorm+SiLU inside the conv's staging) are recorded in EXPERIMENTS.md.
# Fused (flash-style) attention for head dims 32 / 64; MI_FLASH_ATTENTION=0 forces the materialised GEMM + softmax path.
FLASH_ATTENTION = _os.environ.get("MI_FLASH_ATTENTION", "1") == "1"
# GroupNorm statistics from the per-channel sums the producing conv's epilogue emits (no statistics pass over the tensor)
FUSE_GN_STATS = ops.FUSE_GN_STATS


# --------------------------------------------------------------------------------------------- parameters
class ParamArena:
    """All parameters of a network in ONE flat fp32 buffer (+ one for gradients), in an order chosen so that tensors
    the kernels want fused are adjacent (q/k/v weights -> one [3C, C] matrix; every time_emb_proj -> one GEMM).
    The trainable prefix [0, n_trainable) is what the fused optimizer / DDP all-reduce touch; statically unused
    tensors (`proj_attn.*`, never called: UNet:383 vs 418-458) sit behind it and are never updated -- the same
    outcome as torch.optim skipping parameters whose grad is None."""

    def __init__(self, entries, device, late=()):
        # entries: list of (name, shape, trainable); late: names of the trainable tensors whose gradients complete LAST in the
        # backward pass (they must form a prefix of `entries`): [0, n_late) is that prefix, [n_late, n_trainable) the early segment
        # whose data-parallel all-reduce may start at the backward's cut mark (trainer._ArenaTrainer)
        self.offsets, self.shapes = {}, {}
        late = set(late)
        off = 0
        self.n_late = 0
        for trainable_pass in (True, False):
            for name, shape, trainable in entries:
                if trainable != trainable_pass:
                    continue
                n = math.prod(shape)
                self.offsets[name], self.shapes[name] = off, tuple(shape)
                off += n
                if not trainable_pass or n % 4:
                    off = (off + 3) // 4 * 4
                if trainable_pass and name in late:
                    assert self.n_late == self.offsets[name], f"late tensors must form a prefix of the arena ({name})"
                    self.n_late = off
            if trainable_pass:
                off = (off + 3) // 4 * 4
                self.n_trainable = off
        self.numel = max(off, 4)
        self.data = torch.zeros(self.numel, dtype=F32, device=device)
        self.grad = torch.zeros(self.numel, dtype=F32, device=device)

    def view(self, name, flat=None):
        flat = self.data if flat is None else flat
        o, s = self.offsets[name], self.shapes[name]
        return flat[o:o + math.prod(s)].view(s)

    def gview(self, name):
        return self.view(name, self.grad)

    def span(self, names, flat=None):
        """Contiguous view covering consecutive tensors `names` (asserts adjacency)."""
        flat = self.data if flat is None else flat
        o = self.offsets[names[0]]
        end = o
        for nme in names:
            assert self.offsets[nme] == end, f"{nme} is not adjacent in the arena"
            end += math.prod(self.shapes[nme])
        return flat[o:end]


# --------------------------------------------------------------------------------------------- tape
def CUT():
    """Tape marker (a no-op when called): recorded by a model at the forward position behind which -- in backward order: before
    which -- every gradient of the arena's early segment is final.  trainer._ArenaTrainer splits the backward there."""


class Tape:
    def __init__(self):
        self.fns = []
        self.grads = {}
        self.keep = []  # tensors whose id() is used as a key must stay alive

    def record(self, fn):
        self.fns.append(fn)

    # A tensor with two consumers (a ResnetBlock input: norm1 path + residual; a skip: next layer + its slice of d(concat)) collects
    # its gradient branches here.  Two branches stay a PAIR: the GroupNorm backward that consumes them (take2) sums them in fp32 inside
    # its own pass (mi_gn_bwd add / add2) -- the separate add kernel of a skip at 128^3 cost 77 us plus 65-79 us to densify the concat
    # slice first.  Anyone else (take) gets the sum; a third branch folds the pair.
    def take(self, t):
        g = self.grads.pop(id(t), None)
        return ops.add(g[0], g[1]) if isinstance(g, tuple) else g

    def take2(self, t):
        """(branch, second branch or None) -- for consumers that can add two streams themselves."""
        g = self.grads.pop(id(t), None)
        return g if isinstance(g, tuple) else (g, None)

    def put(self, t, g):
        """grad(t) += g."""
        cur = self.grads.get(id(t))
        if cur is None:
            self.grads[id(t)] = g
        elif isinstance(cur, tuple):
            self.grads[id(t)] = ops.add(ops.add(cur[0], cur[1]), g)
        else:
            self.grads[id(t)] = (cur, g)
        self.keep.append(t)

    def move(self, t, other: "Tape"):
        """Hand t's pending gradient (a pair stays a pair) to another tape."""
        g = self.grads.pop(id(t), None)
        if g is not None:
            other.grads[id(t)] = g
            other.keep.append(t)

    def backward(self, out, dout):
        self.put(out, dout)
        for fn in reversed(self.fns):
            fn()
        self.fns.clear()


class Ctx:
    """One forward/backward of one network: parameter views, plan cache, tape."""

    def __init__(self, arena: ParamArena, plans: dict, grad_enabled=True, prepacked=()):
        self.arena, self.plans = arena, plans
        self.tape = Tape() if grad_enabled else None
        self.packed = set(prepacked)  # plan keys whose weights are already packed for this pass (PackBatch.run)
        # algorithmic matmul-class flops of this pass (2*MACs; torch.utils.flop_counter convention)
        self.flops_fwd = 0
        self.flops_bwd = 0
        # id(tensor) -> (ChannelSums, weakref(tensor)): per-channel sums the producing conv emitted, so that the GroupNorm consuming
        # the tensor skips its statistics pass; id(concatenation) -> (a, b, weakref(cat)) lets a GroupNorm over a concat use both
        # halves' sums.  The keys are ids of tensors these dicts do NOT keep alive (a no-grad pass frees activations as it goes and
        # CPython reuses ids), so every lookup checks that the weak reference still IS the tensor asked about.
        self.sums = {}
        self.cat_parts = {}

    def sums_of(self, x):
        ent = self.sums.get(id(x))
        return ent[0] if ent is not None and ent[1]() is x else None

    def parts_of(self, x):
        ent = self.cat_parts.get(id(x))
        return ent[:2] if ent is not None and ent[2]() is x else None

    def count(self, fwd_flops, dgrad=True, wgrad=True):
        self.flops_fwd += fwd_flops
        if self.tape is not None:
            self.flops_bwd += fwd_flops * (int(dgrad) + int(wgrad))

    def p(self, name):
        return self.arena.view(name)

    def g(self, name):
        return self.arena.gview(name)


class PackBatch:
    """Every conv plan of a network re-packed by ONE kernel launch (the weights change every optimizer step; 67 per-conv
    launches are mostly launch floor).  Built once all plans exist, i.e. after a first pass."""

    def __init__(self, arena: ParamArena, plans: dict):
        import ctypes as C
        self.keys = tuple(plans)
        n = len(self.keys)
        plan_arr = (C.c_void_p * n)(*[plans[k].handle for k in self.keys])
        w_arr = (C.c_void_p * n)(*[arena.view(k[0] + ".weight").data_ptr() for k in self.keys])
        h = C.c_void_p()
        _lib.call_raw("mi_conv_pack_batch_create", C.byref(h), plan_arr, w_arr, n)
        self.handle = h

    def run(self):
        call("mi_conv_pack_batch_run", self.handle)
        return self.keys

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.call_raw("mi_conv_pack_batch_destroy", self.handle)
                self.handle = None
        except Exception:
            pass


# --------------------------------------------------------------------------------------------- ops
def gn(ctx: Ctx, x, name, groups, eps):
    """Statistics only; the affine(+SiLU) is applied by the consumer (conv or gn_act)."""
    gamma, beta = ctx.p(name + ".weight"), ctx.p(name + ".bias")
    st = None
    if FUSE_GN_STATS:
        n, v = x.shape[0], x.shape[1] * x.shape[2] * x.shape[3]
        ent, parts = ctx.sums_of(x), ctx.parts_of(x)
        if ent is not None:
            st = ops.gn_stats_from_sums(ent, None, n, v, groups, eps, gamma, beta)
        elif parts is not None:
            ea, eb = ctx.sums_of(parts[0]), ctx.sums_of(parts[1])
            if ea is not None and eb is not None:
                st = ops.gn_stats_from_sums(ea, eb, n, v, groups, eps, gamma, beta)
    if st is None:
        st = ops.gn_stats(x, groups, eps, gamma, beta)
    st.name = name
    return st


# Upsample (nearest x2 on all three axes) + k3 p1 conv as ONE op on the phase kernels (csrc/convph.hip: 8 taps per output voxel on
# the coarse tensor instead of 27 on an up-sampled copy); MI_UPCONV=0: upsample kernel, then the plain conv (A/B runs).
UPCONV = _os.environ.get("MI_UPCONV", "1") == "1"
# MI_CONV1X1=0 (A/B runs) takes 1x1 convs off the streaming kernel, and with it the skip conv's fused forms (resnet)
SKIP_STREAM = _os.environ.get("MI_CONV1X1", "1") != "0"


def upsample_conv(ctx: Ctx, x, name, factors, kernel, padding, out=None):
    """Upsample.forward (UNet:569-588, AEKL Upsample): F.interpolate(x, scale_factor=factors, mode="nearest") then the stride-1 conv
    `name` (kernel, padding).  Fused when the layer is the 3-D factor-2 / k3 / padding-1 case every planner-generated config has."""
    n, d, h, w, cin = x.shape
    fused = UPCONV and tuple(factors) == (2, 2, 2) and tuple(kernel) == (3, 3, 3) and tuple(padding) == (1, 1, 1) and d > 1 and \
        cin % 8 == 0 and ctx.p(name + ".weight").shape[0] % 8 == 0 and x.is_contiguous()
    if not fused:
        return conv(ctx, upsample(ctx, x, factors), name, kernel, (1, 1, 1), padding, out=out)
    return conv(ctx, x, name, kernel, (1, 1, 1), padding, out=out, upconv=True)


def conv_transpose(ctx: Ctx, x, name, kernel, stride, padding):
    """AE Upsample(use_convtranspose=True) (AEKL:66-77): monai's Convolution(is_transposed=True) = nn.ConvTranspose3d(kernel, stride,
    padding, output_padding = stride - 1), weight `name.weight` [Cin, Cout, k, k, k].  A transposed convolution is the data gradient of
    the convolution C: z -> u with the same weight tensor read as [Cout_C = Cin, Cin_C = Cout]: forward = C's dgrad (the phase kernels
    of a k3 s2 p1 conv write the twice finer grid directly), input gradient = C's forward, weight gradient = C's wgrad with (dy, x) in
    the roles of (input, output gradient).  The bias rides in one affine pass over the output.  Supported: 3-D, kernel 3, padding 1,
    stride 2 (or 1) on all axes -- what per-level (stride, kernel, padding) triples of compute_downsample_parameters (CFG:751-797) give."""
    n, d, h, w, cin = x.shape
    wt = ctx.p(name + ".weight")  # [Cin, Cout, 3, 3, 3]
    cout = wt.shape[1]
    k, s_, p_ = tuple(kernel), tuple(stride), tuple(padding)
    if d <= 1 or k != (3, 3, 3) or p_ != (1, 1, 1) or s_ not in ((1, 1, 1), (2, 2, 2)) or cin % 8 or cout % 8:
        raise NotImplementedError(f"use_convtranspose: kernel {k} stride {s_} padding {p_} ({cin}->{cout}) is not on the HIP path "
                                  "(3-D, kernel 3, padding 1, stride 1 or 2 on all axes, channels in multiples of 8)")
    fine = tuple(v * s_[0] for v in (d, h, w))  # output_padding = stride - 1: exactly stride x the input extent
    key = (name, n, d, h, w)
    plan = ctx.plans.get(key)
    if plan is None:
        plan = ctx.plans[key] = ops.ConvPlan(n, fine, cout, cin, k, s_, p_)  # the convolution C on the fine grid: Cout -> Cin channels
    if key not in ctx.packed:
        plan.pack(wt)
        ctx.packed.add(key)
    y0 = plan.dgrad(x)
    bias = ctx.p(name + ".bias")
    ss = torch.stack([torch.ones_like(bias), bias], dim=1).unsqueeze(0).expand(n, cout, 2).contiguous()
    y = ops.gn_apply(y0, ops.GNStats(ss, None, 1), False)  # y = 1 * y0 + bias
    del y0
    ctx.count(2 * y.numel() * cin * 27 // (s_[0] ** 3), dgrad=True)
    if ctx.tape is not None:
        tape = ctx.tape

        def bwd():
            dy = tape.take(y)
            if dy is None:
                return
            plan.wgrad(dy, x, ctx.g(name + ".weight"))
            ops.colsum(dy.contiguous(), out=ctx.g(name + ".bias"), accumulate=True, merge_batch=True)
            tape.put(x, plan.fwd(dy))

        tape.record(bwd)
    return y


def _conv_plan(ctx: Ctx, x, name, kernel, stride, padding, upconv=False):
    """The conv's plan for this input shape, its weights packed for this pass."""
    n, d, h, w, cin = x.shape
    wt = ctx.p(name + ".weight")
    key = (name, n, d, h, w)
    plan = ctx.plans.get(key)
    if plan is None:
        plan = ctx.plans[key] = ops.UpConvPlan(n, (d, h, w), cin, wt.shape[0]) if upconv else ops.ConvPlan(n, (d, h, w), cin, wt.shape[0], kernel, stride, padding)
    if key not in ctx.packed:
        plan.pack(wt)  # [Cout, Cin, (kd,) kh, kw] contiguous: same memory layout for 2-D and 3-D nets
        ctx.packed.add(key)
    return plan


def conv(ctx: Ctx, x, name, kernel, stride, padding, norm=None, silu=False, addvec=None, res=None, d_addvec=None,
         need_dx=True, bias_grad_like=None, out=None, upconv=False, xin=None, y=None, skip=None, park=None):
    """y = conv(act(x)) + addvec + res   (weight `name.weight`, bias folded into addvec by the caller or taken from
    `name.bias` when addvec is None).  norm: GNStats of x, applied (+ SiLU) by one gn_apply pass in front of the conv.
    d_addvec: fp32 [N, Cout] view that receives the per-sample column sums of dy (time-embedding gradient) in backward.
    bias_grad_like: name of a conv whose output gradient is THIS conv's output gradient (a shortcut conv added as `res` of
    that conv): its bias gradient, already computed when this backward runs, is copied instead of reducing dy a second time.
    The ResnetBlock skip conv fused with norm1 (resnet(); csrc/conv1x1.hip) uses four more arguments.  On conv1: xin = act(norm(x)) as
    the skip conv's forward already produced it (no gn_apply pass here); skip = the cell in which the skip conv's backward parks its
    output gradient, so that the norm's backward computes the skip conv's data gradient on the fly.  On the skip conv: y = its output,
    already computed; park = that cell (its backward then runs the weight gradient only)."""
    n, d, h, w, cin = x.shape
    cout = ctx.p(name + ".weight").shape[0]
    plan = _conv_plan(ctx, x, name, kernel, stride, padding, upconv)
    av = addvec if addvec is not None else ctx.p(name + ".bias")
    if xin is None:
        xin = ops.gn_apply(x, norm, silu) if norm is not None else x
    if y is None:
        y, sums = plan.fwd(xin, addvec=av, res=res, out=out, want_sums=True)  # out: channel-slice view of the consumer's concat buffer
        if sums is not None:
            ctx.sums[id(y)] = (sums, weakref.ref(y))
    ctx.count(2 * y.numel() * cin * math.prod(kernel), dgrad=need_dx)
    if ctx.tape is not None:
        tape = ctx.tape

        def bwd():
            dy = tape.take(y)
            if dy is None:
                if skip is not None and "dout" in skip:  # nobody consumes the norm's backward: the parked skip gradient still counts
                    tape.put(x, skip.pop("plan").dgrad(skip.pop("dout")))
                return
            gw = ctx.g(name + ".weight")
            # column sums of dy come out of the wgrad kernel (one extra MFMA per k-step on the dY fragments it holds anyway):
            # per image into `d_addvec` (time-embedding gradient; the caller folds the rows into the bias gradient), or --
            # row pitch 0 -- summed over the batch straight into the bias gradient
            if bias_grad_like is not None:
                plan.wgrad(xin, dy, gw)
                ops.add_f32_(ctx.g(name + ".bias"), ctx.g(bias_grad_like + ".bias"))
            else:
                plan.wgrad(xin, dy, gw, colsum=d_addvec if d_addvec is not None else ctx.g(name + ".bias"))
            if res is not None:
                tape.put(res, dy)
            if park is not None:  # the data gradient is left to the backward of norm1, which runs next
                park["dout"], park["plan"] = dy, plan
            elif need_dx:
                g = plan.dgrad(dy)
                if norm is not None:
                    dout, splan = (skip.pop("dout", None), skip.pop("plan", None)) if skip is not None else (None, None)
                    pending = tape.grads.get(id(x))
                    if dout is not None and (isinstance(pending, tuple) or not ops.skip_fusable(2, splan, dout, g, x, pending)):
                        tape.put(x, splan.dgrad(dout))  # a third branch, or pitches the kernel refuses: the skip gradient as a tensor
                        dout = None
                    if dout is not None:
                        other = tape.take(x)
                        dx = ops.conv1x1_dgrad_gn_bwd(splan, dout, g, x, norm, ctx.p(norm.name + ".weight"), ctx.g(norm.name + ".weight"),
                                                      ctx.g(norm.name + ".bias"), add2=other)
                    else:
                        other, other2 = tape.take2(x)
                        dx = ops.gn_bwd(g, x, norm, ctx.p(norm.name + ".weight"), silu, ctx.g(norm.name + ".weight"),
                                        ctx.g(norm.name + ".bias"), add=other, add2=other2)
                    tape.grads[id(x)] = dx
                    tape.keep.append(x)
                else:
                    tape.put(x, g)

        tape.record(bwd)
    return y


def upsample(ctx: Ctx, x, factors):
    y = ops.upsample_nearest(x, factors)
    if ctx.tape is not None:
        tape = ctx.tape

        def bwd():
            dy = tape.take(y)
            if dy is not None:
                tape.put(x, ops.upsample_nearest_bwd(ops.dense(dy), factors))  # dy may be a slice view of d(concat)

        tape.record(bwd)
    return y


def checkpoint(ctx: Ctx, fn, x):
    """Activation checkpointing at tape level (the torch.utils.checkpoint of autoencoderkl_with_strides.py:761-762, 815-816, also
    offered per block for the U-Net): y = fn(ctx', x) runs WITHOUT a tape, so every intermediate of the segment is freed as soon
    as its consumer has run; the recorded backward re-runs fn with a tape and back-propagates through it.  The recomputation
    launches the same kernels on the same inputs, and the segment input's pending gradient is handed to the inner tape so that
    the fused "+ other branch" of the GroupNorm backward sees what it would have seen: gradients are bit-identical to the
    stored-activation path (tests/test_checkpoint_gpu.py).  Recomputed flops are not counted (SURVEY 8d convention)."""
    if ctx.tape is None:
        return fn(ctx, x)
    sub = Ctx(ctx.arena, ctx.plans, grad_enabled=False)
    sub.packed, sub.sums, sub.cat_parts = ctx.packed, ctx.sums, ctx.cat_parts  # same packed weights, same emitted channel sums
    y = fn(sub, x)
    ctx.flops_fwd += sub.flops_fwd
    ctx.flops_bwd += 2 * sub.flops_fwd
    tape = ctx.tape

    def bwd():
        dy = tape.take(y)
        if dy is None:
            return
        inner = Ctx(ctx.arena, ctx.plans, grad_enabled=True)
        inner.packed, inner.sums, inner.cat_parts = ctx.packed, ctx.sums, ctx.cat_parts
        y2 = fn(inner, x)
        it = inner.tape
        tape.move(x, it)  # (a pending pair stays a pair: the inner GroupNorm backward must see what the stored-activation path sees)
        it.backward(y2, dy)
        g = it.take(x)
        if g is not None:
            tape.grads[id(x)] = g
            tape.keep.append(x)
        it.grads.clear(), it.keep.clear()

    tape.record(bwd)
    return y


def avg_pool(ctx: Ctx, x, kernel, stride):
    """Pool[AVG](kernel_size, stride) of Downsample(use_conv=False) (UNet:522)."""
    y = ops.avg_pool(x, kernel, stride)
    if ctx.tape is not None:
        tape = ctx.tape
        dims = tuple(x.shape[1:4])

        def bwd():
            dy = tape.take(y)
            if dy is not None:
                tape.put(x, ops.avg_pool_bwd(ops.dense(dy), dims, kernel, stride))

        tape.record(bwd)
    return y


def gn_act(ctx: Ctx, x, st, silu):
    """act(GroupNorm(x)) as a tensor of its own (for consumers other than a conv, which applies its own norm: the resamplers of
    ResnetBlock(up / down), UNet:679-687).  Backward folds the other gradient branches of x in, like conv's backward."""
    y = ops.gn_apply(x, st, silu)
    if ctx.tape is not None:
        tape = ctx.tape

        def bwd():
            g = tape.take(y)
            if g is None:
                return
            other, other2 = tape.take2(x)
            dx = ops.gn_bwd(g, x, st, ctx.p(st.name + ".weight"), silu, ctx.g(st.name + ".weight"), ctx.g(st.name + ".bias"),
                            add=other, add2=other2)
            tape.grads[id(x)] = dx
            tape.keep.append(x)

        tape.record(bwd)
    return y


def add(ctx: Ctx, a, b, b_needs_grad=True):
    """a + b (ControlNet residual inputs, UNet:1995-2010)."""
    y = ops.add(a, b)
    if ctx.tape is not None:
        tape = ctx.tape

        def bwd():
            dy = tape.take(y)
            if dy is not None:
                tape.put(a, dy)
                if b_needs_grad:
                    tape.put(b, dy)

        tape.record(bwd)
    return y


# The 1x1 skip conv of a ResnetBlock shares its passes over x with norm1 (csrc/conv1x1.hip): True (both directions), False, or "fwd" /
# "bwd" (one of them: measurements).  resnet(fuse_skip=) overrides it per call (tests compare the routes).
SKIP_FUSE = True


def resnet(ctx: Ctx, x, name, sd, groups, eps, addvec, d_addvec, mode=None, stride=None, kernel=None, out=None, fuse_skip=None):
    """ResnetBlock.forward (UNet:674-701): 2 statistics passes (mostly from the producing convs' epilogues) + 3 fused convs.
    addvec: fp32 [N, Cout] = time_emb_proj(silu(emb)) + conv1.bias; d_addvec receives conv1's per-image dy column sums.
    mode: None | 'up' (nearest x stride) | 'down' (avg-pool kernel/stride): both x and act(norm1(x)) are resampled (UNet:679-687).
    out: where conv2 writes the block's result (the first channels of the next skip-concat buffer).
    fuse_skip (default SKIP_FUSE): a block with a skip conv and no resampling runs the skip conv first -- its kernel reads x once and
    also writes act(norm1(x)) for conv1 -- and in backward leaves the skip conv's data gradient to norm1's backward apply, where the
    streaming 1x1 kernel covers the shape (ops.skip_fusable); every other block takes the separate passes."""
    k3, s1, p1 = (1,) * (3 - sd) + (3,) * sd, (1, 1, 1), (0,) * (3 - sd) + (1,) * sd
    name = name + "." if name else ""  # stand-alone blocks (blocks.ResnetBlock) have un-prefixed parameter names
    n1 = gn(ctx, x, name + "norm1", groups, eps)
    has_skip = name + "skip_connection.conv.weight" in ctx.arena.offsets
    fuse = SKIP_FUSE if fuse_skip is None else fuse_skip
    xs = a1 = cell = None
    if fuse and mode is None and has_skip and SKIP_STREAM and n1._pending is None:
        splan = _conv_plan(ctx, x, name + "skip_connection.conv", (1, 1, 1), s1, (0, 0, 0))
        if fuse in (True, "fwd") and ops.skip_fusable(1, splan, x):
            xs, a1 = ops.conv1x1_fwd_gn_apply(splan, x, n1, ctx.p(name + "skip_connection.conv.bias"))
        if fuse in (True, "bwd") and ctx.tape is not None and ops.skip_fusable(2, splan, x):
            cell = {}
    if mode is None:
        h = conv(ctx, x, name + "conv1.conv", k3, s1, p1, norm=n1, silu=True, addvec=addvec, d_addvec=d_addvec, xin=a1, skip=cell)
    else:
        h = gn_act(ctx, x, n1, True)
        if mode == "up":
            x, h = upsample(ctx, x, stride), upsample(ctx, h, stride)
        else:
            x, h = avg_pool(ctx, x, kernel, stride), avg_pool(ctx, h, kernel, stride)
        h = conv(ctx, h, name + "conv1.conv", k3, s1, p1, addvec=addvec, d_addvec=d_addvec)
    n2 = gn(ctx, h, name + "norm2", groups, eps)
    if has_skip:  # (recorded here, behind conv1, whichever route: its backward runs before conv1's)
        xs = conv(ctx, x, name + "skip_connection.conv", (1, 1, 1), s1, (0, 0, 0), bias_grad_like=name + "conv2.conv", y=xs, park=cell)
    else:
        xs = x
    return conv(ctx, h, name + "conv2.conv", k3, s1, p1, norm=n2, silu=True, res=xs, out=out)


def concat_buffer(a_shape, ca, cb, device):
    """Allocate the [.., ca + cb] buffer of an upcoming `concat(a, b)` and return (buffer, view of its first ca channels): the
    producer of `a` writes there directly (conv `out=`), so that half of the concatenation costs nothing."""
    buf = torch.empty(tuple(a_shape[:-1]) + (ca + cb,), dtype=BF16, device=device)
    return buf, buf[..., :ca]


def concat(ctx: Ctx, a, b, buf=None):
    """torch.cat([a, b], channel axis) (UNet:1263, 1377, 1504).  buf: the concatenation's buffer when one or both halves already
    live in it -- `a` written there by its producing conv (concat_buffer), `b` (the skip) written there when it was produced
    (unet._run: skip slots).  Only the halves that are elsewhere are copied; in backward the gradient of an in-place half is a
    channel-slice VIEW of d(cat), not a copy."""
    ca, cb = a.shape[-1], b.shape[-1]
    a_in = buf is not None and a.data_ptr() == buf.data_ptr() and ops._cs(a) == ca + cb
    b_in = buf is not None and b.data_ptr() == buf.data_ptr() + 2 * ca and ops._cs(b) == ca + cb
    if a_in or b_in:
        n, v = a.shape[0], a.shape[1] * a.shape[2] * a.shape[3]
        if not a_in:
            call("mi_copy_channels", ptr(a), ops._cs(a), 0, ptr(buf), ca + cb, 0, ca, n * v)
        if not b_in:
            call("mi_copy_channels", ptr(b), ops._cs(b), 0, ptr(buf), ca + cb, ca, cb, n * v)
        y = buf
    else:
        y = ops.concat_channels(a, b)
    ctx.cat_parts[id(y)] = (a, b, weakref.ref(y))
    if ctx.tape is not None:
        tape = ctx.tape

        def bwd():
            dy = tape.take(y)
            if dy is None:
                return
            for t, lo, n_c, in_place in ((a, 0, ca, a_in), (b, ca, cb, b_in)):
                if in_place and id(t) not in tape.grads:  # first gradient of this half: hand the slice over as a strided view
                    tape.grads[id(t)] = dy[..., lo:lo + n_c]
                    tape.keep.append(t)
                    tape.keep.append(dy)
                else:
                    tape.put(t, ops.slice_channels(dy, lo, n_c))

        tape.record(bwd)
    return y


def token_wgrad(dy, x, out=None):
    """dW [N, K] = dy^T x, reduced over the token rows of dy [M, N] and x [M, K] (bf16): both are transposed to a token-last pitch rounded
    up to 8 (pad columns zeroed by the transpose kernel), then one GEMM runs over it.  out: fp32 view to ACCUMULATE into (else returned)."""
    return ops.gemm_nt(ops.transpose(dy, pad_to=8), ops.transpose(x, pad_to=8), out=out, out_f32=True, accumulate=out is not None)


def linear_dgrad(dy, wb, out_f32=False):
    """dx [M, K] = dy [M, N] @ W for the bf16 weight W [N, K]: one transpose of W, one GEMM."""
    return ops.gemm_nt(dy, ops.transpose(wb), out_f32=out_f32)


def _heads(t, b, heads):
    """[B * S, C] token matrix, a column block of a wider one, or a dense [B, D, H, W, C] activation -> its head views [B, heads, S, hd]."""
    return t.view(b, -1, heads, t.shape[-1] // heads).permute(0, 2, 1, 3)


def _sdpa(q, k, v, scale, out, res=None):
    """out = softmax(q k^T * scale) v (+ res) per head with materialised fp32 scores (head widths the fused kernels do not take; query and
    key/value token counts may differ).  q, out, res [B, heads, Sq, hd], k / v [B, heads, Skv, hd]: views (_heads).  Every bf16 matrix whose
    LAST axis is a token axis is a GEMM operand reduced over that axis: the NT GEMM loads 16-byte pieces along K, so those matrices get
    a row pitch rounded up to a multiple of 8 with zero pad columns (written by the softmax / transpose kernels themselves) and the
    products run over the padded K.  (3^3 = 27 or 5^3 = 125 tokens at the coarsest level of non-power-of-two patches.)
    Returns backward(do, dq, dk, dv), which writes the three gradients into the views it is given."""
    if q.shape[-1] % 8:
        raise ValueError("head width must be a multiple of 8 on the HIP path")
    scores = ops.gemm_nt(q, k, alpha=scale, out_f32=True)                         # [B, heads, Sq, Skv]
    probs = ops.softmax_fwd(scores, pad8=True)                                    # ... view, pitch Skv rounded up to 8
    del scores
    ops.gemm_nt(ops.padded(probs), ops.transpose(v, pad_to=8), out=out, res=res)

    def bwd(do, dq, dk, dv):
        dp = ops.gemm_nt(do, v, out_f32=True)
        ds = ops.softmax_bwd(probs, dp, scale)                                    # [B, heads, Sq, Skv] view, padded pitch
        del dp
        ops.gemm_nt(ops.padded(ds), ops.transpose(k, pad_to=8), out=dq)
        qt = ops.transpose(q, pad_to=8)                                           # [B, heads, hd, Sq rounded up to 8]
        dst = ops.transpose(ds, pad_to=8)                                         # dS^T [B, heads, Skv, ...]
        ops.gemm_nt(dst, qt, out=dk)
        del dst, ds
        pt = ops.transpose(probs, pad_to=8)                                       # P^T
        ops.gemm_nt(pt, ops.transpose(do, pad_to=8), out=dv)

    return bwd


def _attention_flash(ctx, x, name, st, xn, wqkv, qkv, b, s, c, heads, scale):
    """Head dims 32 / 64: fused attention kernels (csrc/attention.hip); the projections stay on the NT GEMM."""
    dev = x.device
    d_, h_, w_ = x.shape[1:4]
    y = torch.empty_like(x)
    lse = torch.empty((b * heads, s), dtype=F32, device=dev)
    nws = _lib.call_raw("mi_attn_workspace_bytes", c, heads, b, s)
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=dev)  # partial results of the split kernels; dead after each call
    call("mi_attn_fwd", ptr(qkv), 3 * c, c, heads, b, s, float(scale), ptr(x), ptr(y), ptr(lse), ptr(ws), nws)
    del ws
    ctx.count(2 * b * s * c * 3 * c)
    ctx.count(4 * b * s * s * c)
    if ctx.tape is not None:
        tape = ctx.tape

        def bwd():
            dy = tape.take(y)
            if dy is None:
                return
            dqkv = torch.empty((b * s, 3 * c), dtype=BF16, device=dev)
            dsum = torch.empty((b * heads, s), dtype=F32, device=dev)
            ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=dev)
            call("mi_attn_bwd", ptr(qkv), 3 * c, c, heads, b, s, float(scale), ptr(y), ptr(x), ptr(dy), ptr(lse), ptr(dsum), ptr(dqkv),
                 ptr(ws), nws)
            _attention_param_and_input_grads(ctx, tape, x, name, st, xn, wqkv, dqkv, dy, b, s, c)

        tape.record(bwd)
    return y


def _attention_param_and_input_grads(ctx, tape, x, name, st, xn, wqkv, dqkv, dy, b, s, c):
    """Shared tail of the attention backward: projection weight/bias gradients, dx through the projections and the norm."""
    pre = name + "." if name else ""
    gw = ctx.arena.span([f"{pre}to_{t}.weight" for t in "qkv"], ctx.arena.grad)
    gb = ctx.arena.span([f"{pre}to_{t}.bias" for t in "qkv"], ctx.arena.grad)
    # dW[3C, C] += dqkv^T xn and db += colsum(dqkv) in ONE pass over the two activations (no transposes, no long-K GEMM on 12 workgroups)
    call("mi_linear_wgrad_bf16", ptr(xn), c, c, ptr(dqkv), 3 * c, 3 * c, b * s, ptr(gw), ptr(gb))
    dxn = linear_dgrad(dqkv, wqkv).view(x.shape)
    other = tape.take(x)
    dx = ops.gn_bwd(dxn, x, st, ctx.p(pre + "norm.weight"), False, ctx.g(pre + "norm.weight"), ctx.g(pre + "norm.bias"), add=dy, add2=other)
    tape.grads[id(x)] = dx
    tape.keep.append(x)


def attention(ctx: Ctx, x, name, groups, eps, heads):
    """AttentionBlock.forward (UNet:418-458 / AEKL:283-323): GN -> q,k,v -> softmax(QK^T/sqrt(d)) V -> + x.  No out-proj.
    Channels-last makes the reference's [B,C,S]->[B,S,C] transpose free."""
    b, d_, h_, w_, c = x.shape
    s = d_ * h_ * w_
    scale = 1.0 / math.sqrt(c / heads)
    dev = x.device
    pre = name + "." if name else ""  # stand-alone blocks (blocks.AttentionBlock) have un-prefixed parameter names
    st = gn(ctx, x, pre + "norm", groups, eps)
    xn = ops.gn_apply(x, st, False)                                              # [B, S, C]
    wqkv = ops.cast_bf16(ctx.arena.span([f"{pre}to_{t}.weight" for t in "qkv"]).view(3 * c, c))
    bqkv = ctx.arena.span([f"{pre}to_{t}.bias" for t in "qkv"])
    qkv = ops.gemm_nt(xn.view(b * s, c), wqkv, bias=bqkv)                         # [B*S, 3C]
    if FLASH_ATTENTION and _lib.call_raw("mi_attn_supported", c, heads):
        return _attention_flash(ctx, x, name, st, xn, wqkv, qkv, b, s, c, heads, scale)
    q, k, v = (_heads(qkv[:, i * c:(i + 1) * c], b, heads) for i in range(3))
    y = torch.empty_like(x)
    sdpa_bwd = _sdpa(q, k, v, scale, out=_heads(y, b, heads), res=_heads(x, b, heads))
    ctx.count(2 * b * s * c * 3 * c)       # q, k, v projections
    ctx.count(4 * b * s * s * c)           # QK^T and PV
    if ctx.tape is not None:
        tape = ctx.tape

        def bwd():
            dy = tape.take(y)
            if dy is None:
                return
            dqkv = torch.empty((b * s, 3 * c), dtype=BF16, device=dev)
            sdpa_bwd(_heads(dy, b, heads), *(_heads(dqkv[:, i * c:(i + 1) * c], b, heads) for i in range(3)))
            _attention_param_and_input_grads(ctx, tape, x, name, st, xn, wqkv, dqkv, dy, b, s, c)

        tape.record(bwd)
    return y


def linear_f32(x_f32, w, b, gw, gb):
    """Tiny fp32-in / fp32-out Linear on the embedding vectors (bf16 MFMA inside).  w [out, in], b [out] and their
    gradient buffers gw, gb are fp32 arena views.  Returns (y, backward(dy) -> dx)."""
    xb, wb = ops.cast_bf16(x_f32), ops.cast_bf16(w)
    y = ops.gemm_nt(xb, wb, bias=b, out_f32=True)

    def bwd(dy_f32, need_dx=True):
        """dy may be a column slice; accumulates into the weight/bias gradients, returns dx (fp32) or None."""
        dyb = ops.cast_bf16(dy_f32)
        ops.sum_rows_f32(dy_f32, gb, accumulate=True)
        token_wgrad(dyb, xb, out=gw)
        return linear_dgrad(dyb, wb, out_f32=True) if need_dx else None

    return y, bwd


# --------------------------------------------------------------------------------------------- cross-attention path (UNet:72-342)
def _reshape(ctx: Ctx, x, shape):
    """x viewed with another shape (same storage): channels-last activations ARE the [B*S, C] token matrix (UNet:327-330 for free)."""
    y = x.view(shape)
    if ctx.tape is not None:
        tape = ctx.tape

        def bwd():
            g = tape.take(y)
            if g is not None:
                tape.put(x, ops.dense(g).view(x.shape))

        tape.record(bwd)
    return y


def layernorm(ctx: Ctx, x, name, eps=1e-5):
    """nn.LayerNorm(C) over token rows x [M, C] bf16 (UNet:219-221)."""
    m, c = x.shape
    gamma, beta = ctx.p(name + ".weight"), ctx.p(name + ".bias")
    y = torch.empty_like(x)
    mr = torch.empty((m, 2), dtype=F32, device=x.device)
    call("mi_layernorm_fwd", ptr(x), c, ptr(gamma), ptr(beta), ptr(y), c, ptr(mr), m, c, float(eps))
    if ctx.tape is not None:
        tape = ctx.tape

        def bwd():
            dy = tape.take(y)
            if dy is None:
                return
            dx = torch.empty_like(x)
            call("mi_layernorm_bwd", ptr(dy), c, ptr(x), c, ptr(gamma), ptr(mr), ptr(dx), c, ptr(ctx.g(name + ".weight")),
                 ptr(ctx.g(name + ".bias")), m, c)
            tape.put(x, dx)

        tape.record(bwd)
    return y


def linear(ctx: Ctx, x, name, bias=True, res=None, need_dx=True):
    """nn.Linear on token rows: y = x W^T (+ b) (+ res).  x [M, K] bf16 dense, W fp32 [N, K] in the arena (bf16 MFMA, fp32 accumulate)."""
    m, k = x.shape
    w = ctx.p(name + ".weight")
    n = w.shape[0]
    if k % 8 or n % 8:
        raise ValueError(f"{name}: feature counts must be multiples of 8 on the HIP path (got {k} -> {n})")
    wb = ops.cast_bf16(w)
    y = ops.gemm_nt(x, wb, bias=ctx.p(name + ".bias") if bias else None, res=res)
    ctx.count(2 * m * n * k, dgrad=need_dx)
    if ctx.tape is not None:
        tape = ctx.tape

        def bwd():
            dy = tape.take(y)
            if dy is None:
                return
            call("mi_linear_wgrad_bf16", ptr(x), k, k, ptr(dy), n, n, m, ptr(ctx.g(name + ".weight")), ptr(ctx.g(name + ".bias")) if bias else None)
            if res is not None:
                tape.put(res, dy)
            if need_dx:
                tape.put(x, linear_dgrad(dy, wb))

        tape.record(bwd)
    return y


def geglu(ctx: Ctx, h):
    """GEGLU of monai's MLPBlock(act="GEGLU") (UNet:211): h [M, 2F] -> h[:, :F] * gelu(h[:, F:])."""
    m, f2 = h.shape
    f = f2 // 2
    y = torch.empty((m, f), dtype=BF16, device=h.device)
    call("mi_geglu_fwd", ptr(h), ptr(y), m, f)
    if ctx.tape is not None:
        tape = ctx.tape

        def bwd():
            dy = tape.take(y)
            if dy is not None:
                dh = torch.empty_like(h)
                call("mi_geglu_bwd", ptr(h), ptr(dy), ptr(dh), m, f)
                tape.put(h, dh)

        tape.record(bwd)
    return y


def mha(ctx: Ctx, q, k, v, b, sq, skv, heads):
    """CrossAttention._attention (UNet:135-154): softmax(Q K^T / sqrt(d)) V per head; q [B*Sq, C], k / v [B*Skv, C] bf16 dense, the
    heads are column slices (reshape_heads_to_batch_dim is free in this layout).  Materialised scores (_sdpa): the query and key/value
    token counts differ for a context."""
    c = q.shape[1]
    o = torch.empty((b * sq, c), dtype=BF16, device=q.device)
    sdpa_bwd = _sdpa(*(_heads(t, b, heads) for t in (q, k, v)), 1.0 / math.sqrt(c // heads), out=_heads(o, b, heads))
    ctx.count(4 * b * sq * skv * c)
    if ctx.tape is not None:
        tape = ctx.tape

        def bwd():
            do = tape.take(o)
            if do is None:
                return
            dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
            sdpa_bwd(*(_heads(t, b, heads) for t in (do, dq, dk, dv)))
            tape.put(q, dq), tape.put(k, dk), tape.put(v, dv)

        tape.record(bwd)
    return o


def spatial_transformer(ctx: Ctx, x, name, context, groups, eps, heads, layers):
    """SpatialTransformer.forward (UNet:314-342) with BasicTransformerBlock.forward (UNet:225-234) inlined:
    GroupNorm -> 1x1 proj_in -> [self-attention, cross-attention on `context`, GEGLU feed-forward] x layers -> 1x1 proj_out + x.
    context: bf16 [B * Sc, Cc] token matrix (or None: attn2 is a second self-attention, UNet:159); it is a constant of the step
    (a text / label encoder is trained through its own graph)."""
    b, d_, h_, w_, c = x.shape
    s = d_ * h_ * w_
    pre = name + "." if name else ""
    st = gn(ctx, x, pre + "norm", groups, eps)
    xn = gn_act(ctx, x, st, False)
    one, zero = (1, 1, 1), (0, 0, 0)
    t = _reshape(ctx, conv(ctx, xn, pre + "proj_in.conv", one, one, zero), (b * s, c))
    sc = context.shape[0] // b if context is not None else s
    for li in range(layers):
        blk = f"{pre}transformer_blocks.{li}"
        n1 = layernorm(ctx, t, blk + ".norm1")
        a1 = blk + ".attn1"
        o = mha(ctx, linear(ctx, n1, a1 + ".to_q", bias=False), linear(ctx, n1, a1 + ".to_k", bias=False),
                linear(ctx, n1, a1 + ".to_v", bias=False), b, s, s, heads)
        t = linear(ctx, o, a1 + ".to_out.0", res=t)
        n2 = layernorm(ctx, t, blk + ".norm2")
        a2 = blk + ".attn2"
        kv_src, kv_grad = (context, False) if context is not None else (n2, True)
        o = mha(ctx, linear(ctx, n2, a2 + ".to_q", bias=False), linear(ctx, kv_src, a2 + ".to_k", bias=False, need_dx=kv_grad),
                linear(ctx, kv_src, a2 + ".to_v", bias=False, need_dx=kv_grad), b, s, sc, heads)
        t = linear(ctx, o, a2 + ".to_out.0", res=t)
        n3 = layernorm(ctx, t, blk + ".norm3")
        t = linear(ctx, geglu(ctx, linear(ctx, n3, blk + ".ff.linear1")), blk + ".ff.linear2", res=t)
    return conv(ctx, _reshape(ctx, t, (b, d_, h_, w_, c)), pre + "proj_out.conv", one, one, zero, res=x)
