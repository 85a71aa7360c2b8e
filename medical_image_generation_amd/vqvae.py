"""VQVAE on the MI355X HIP path: the autoencoder both reference trainers build under `--latent_space_type vq`
(medimgen/train_autoencoder.py:50-51, 407-409; medimgen/train_ldm.py:54-58, 85-105).

The class is third-party (`generative.networks.nets.VQVAE`, MONAI-Generative 0.2.x), its source is not under the reference tree: the
constructor keywords, `state_dict()` names (`encoder.blocks.<j>...`, `decoder.blocks.<j>...`, `quantizer.quantizer.*`), methods and
arithmetic here follow upstream as restated in tests/vqvae_ref.py -- PARITY UNPINNED against the original.

Kernels: csrc/vq.hip (nearest code, straight-through gather + commitment loss, its backward, EMA codebook update).  The k3 / s1 / p1
convs run on the conv plans of engine.conv (residual add in the epilogue); every other cubic (kernel, stride, padding) runs on the patch matrix + bf16 NT
GEMM route of the discriminator (mi_im2col3d / mi_col2im3d / mi_gemm_nt_bf16), a ConvTranspose as the data gradient of the matching
conv; ReLU is mi_leaky_relu_* with slope 0.  `encode` and `decode` are one autograd edge each, `quantize` is its own edge with the
straight-through backward."""
from __future__ import annotations

import math

import torch
from torch import nn

from . import engine as E
from . import hipops as ops
from ._lib import call, constants, ptr
from .discriminator import leaky_relu
from .unet import HipModule, ParamSpec, _NetFn

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
MAX_D, MAX_K = 256, 8192


# ------------------------------------------------------------------------------------------------ quantiser ops (csrc/vq.hip)
def _tokens(z_cl):
    """[N, D, H, W, C] channels-last bf16 (dense, or a channel slice of a wider buffer) -> (T, C, pitch)."""
    return math.prod(z_cl.shape[:-1]), z_cl.shape[-1], ops._cs(z_cl)


def ema_workspace_bytes(T: int, K: int) -> int:
    c = constants()
    chunks = max(1, min(c["MI_VQ_EMA_MAX_CHUNKS"], -(-T // c["MI_VQ_EMA_CHUNK"])))
    return 8 + 4 * (chunks * K + 2 * K + T)


def vq_assign(z_cl, codebook):
    """idx int32 [N, D, H, W] = nearest code of every voxel's channel vector."""
    t, d, cs = _tokens(z_cl)
    idx = torch.empty(z_cl.shape[:-1], dtype=I32, device=z_cl.device)
    call("mi_vq_assign", ptr(z_cl), cs, ptr(codebook), ptr(idx), t, d, codebook.shape[0])
    return idx


def vq_gather_loss(z_cl, codebook, idx, commitment_cost, loss=None):
    """-> (zq bf16 like z_cl = z + (q - z), diff fp32 [T, C] = q - z, loss fp32 [1] = commitment_cost * mean((q - z)^2))."""
    t, d, cs = _tokens(z_cl)
    dev = z_cl.device
    zq = torch.empty(z_cl.shape, dtype=BF16, device=dev)
    diff = torch.empty((t, d), dtype=F32, device=dev)
    loss = torch.empty(1, dtype=F32, device=dev) if loss is None else loss
    partials = torch.empty(constants()["MI_VQ_PARTIALS"], dtype=torch.float64, device=dev)
    call("mi_vq_gather_loss", ptr(z_cl), cs, ptr(codebook), ptr(idx), ptr(zq), d, ptr(diff), ptr(loss), ptr(partials), t, d, codebook.shape[0],
         float(commitment_cost))
    return zq, diff, loss


def vq_embed(idx, codebook):
    """bf16 [.., C] = codebook[idx] (int32 indices)."""
    zq = torch.empty(tuple(idx.shape) + (codebook.shape[1],), dtype=BF16, device=idx.device)
    call("mi_vq_gather_loss", None, 0, ptr(codebook), ptr(idx), ptr(zq), codebook.shape[1], None, None, None, idx.numel(), codebook.shape[1],
         codebook.shape[0], 0.0)
    return zq


def vq_bwd(dq_cl, diff, weight, scale):
    """dz = dq + weight[0] * scale * (z - q); weight: fp32 device scalar, scale = 2 * commitment_cost / numel."""
    t, d, cs = _tokens(dq_cl)
    dz = torch.empty(dq_cl.shape, dtype=BF16, device=dq_cl.device)
    call("mi_vq_bwd", ptr(dq_cl), cs, ptr(diff), ptr(weight), float(scale), ptr(dz), d, t, d)
    return dz


def vq_ema_update(z_cl, idx, embedding, ema_cluster_size, ema_w, decay, eps, perplexity):
    t, d, cs = _tokens(z_cl)
    k = embedding.shape[0]
    nbytes = ema_workspace_bytes(t, k)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=z_cl.device)
    call("mi_vq_ema_update", ptr(z_cl), cs, ptr(idx), t, d, k, ptr(embedding), ptr(ema_cluster_size), ptr(ema_w), float(decay), float(eps),
         ptr(perplexity), ptr(ws), nbytes)


# ------------------------------------------------------------------------------------------------ convs on the patch-matrix route
def _up8(n):
    return (n + 7) // 8 * 8


def _gemm_channels(c, taps):
    """Channels of the tensor that goes through mi_im2col3d: the GEMM reduces over taps * channels, a multiple of 8."""
    return c if (taps * c) % 8 == 0 else _up8(c)


def _fit(x, c_to):
    """x [.., C] -> dense [.., c_to]: the first channels, zero-filled from C on."""
    nvox = math.prod(x.shape[:-1])
    y = torch.empty(tuple(x.shape[:-1]) + (c_to,), dtype=BF16, device=x.device)
    call("mi_fit_channels_bf16", ptr(x), ops._cs(x), x.shape[-1], ptr(y), c_to, nvox)
    return y


def _pack(wt, co, ci, cip, taps):
    """torch weight [co, ci, taps] -> (w2 [co, taps * cip], w2t [taps * cip, co]) bf16, input channels zero-padded to cip."""
    dev = wt.device
    if cip != ci:
        wp = torch.empty((co, cip, taps), dtype=F32, device=dev)
        call("mi_pad_cin_f32", ptr(wt), ptr(wp), co, ci, cip, taps)
        wt = wp
    w2 = torch.empty((co, taps * cip), dtype=BF16, device=dev)
    w2t = torch.empty((taps * cip, co), dtype=BF16, device=dev)
    call("mi_disc_pack_weights", ptr(wt), ptr(w2), ptr(w2t), co, co, cip, taps)
    return w2, w2t


def _unpack_wgrad(dw2, gw, co, ci, cip, taps):
    """gw [co, ci, taps] += dw2 [co, taps * cip] (the pad channels' rows dropped)."""
    if cip == ci:
        call("mi_disc_wgrad_unpack", ptr(dw2), ptr(gw), co, ci, taps)
        return
    tmp = torch.empty((co, cip * taps), dtype=F32, device=dw2.device)
    ops.zero_f32_2d_(tmp)
    call("mi_disc_wgrad_unpack", ptr(dw2), ptr(tmp), co, cip, taps)
    ops.add_f32_(gw.view(co, ci * taps), tmp[:, :ci * taps])


def _bias_grad(ctx: E.Ctx, name, dy):
    """`name.bias` gradient += column sums of dy [.., C] (dense) in a fixed summation order (ops.colsum and the conv weight-gradient
    kernel's column sums add workgroup totals with float atomics)."""
    c = dy.shape[-1]
    rows = dy.numel() // c
    k = constants()
    chunks = min(k["MI_VQ_COLSUM_MAX_CHUNKS"], -(-rows // k["MI_VQ_COLSUM_ROWS"]))
    ws = torch.empty(chunks * c, dtype=torch.float64, device=dy.device)
    call("mi_colsum_det_bf16", ptr(dy), c, rows, c, ptr(ctx.g(name + ".bias")), ptr(ws))


K3, S1, P1 = (3, 3, 3), (1, 1, 1), (1, 1, 1)


def conv_k3(ctx: E.Ctx, x, name, res=None, need_dx=True):
    """y = conv(x) + bias (+ res) for kernel 3 / stride 1 / padding 1 on the conv plans (engine.conv without its GroupNorm plumbing; the
    bias gradient comes from _bias_grad)."""
    plan = E._conv_plan(ctx, x, name, K3, S1, P1)
    y = plan.fwd(x, addvec=ctx.p(name + ".bias"), res=res)
    ctx.count(2 * y.numel() * x.shape[-1] * 27, dgrad=need_dx)
    if ctx.tape is not None:
        tape = ctx.tape

        def bwd():
            dy = tape.take(y)
            if dy is None:
                return
            dy = ops.dense(dy)
            plan.wgrad(x, dy, ctx.g(name + ".weight"))
            _bias_grad(ctx, name, dy)
            if res is not None:
                tape.put(res, dy)
            if need_dx:
                tape.put(x, plan.dgrad(dy))

        tape.record(bwd)
    return y


def conv_gemm(ctx: E.Ctx, x, name, k, s, p, need_dx=True):
    """nn.Conv3d(kernel k, stride s, padding p) with bias on NDHWC bf16, weight `name.weight` [Cout, Cin, k, k, k], Cout % 8 == 0."""
    n, d, h, w, cin = x.shape
    wt = ctx.p(name + ".weight")
    cout, taps = wt.shape[0], k * k * k
    cip = _gemm_channels(cin, taps)
    do, ho, wo = ((v + 2 * p - k) // s + 1 for v in (d, h, w))
    m, kk, dev = n * do * ho * wo, taps * cip, x.device
    w2, w2t = _pack(wt, cout, cin, cip, taps)
    xs = _fit(x, cip) if cip != cin else ops.dense(x)
    patches = torch.empty((m, kk), dtype=BF16, device=dev)
    call("mi_im2col3d", ptr(xs), cip, ptr(patches), n, d, h, w, cip, k, s, p)
    y = ops.gemm_nt(patches, w2, bias=ctx.p(name + ".bias")).view(n, do, ho, wo, cout)
    ctx.count(2 * m * cout * taps * cin, dgrad=need_dx)
    if ctx.tape is not None:
        tape = ctx.tape

        def bwd():
            dy = tape.take(y)
            if dy is None:
                return
            dy = ops.dense(dy)
            _bias_grad(ctx, name, dy)
            _unpack_wgrad(E.token_wgrad(dy.view(m, cout), patches), ctx.g(name + ".weight"), cout, cin, cip, taps)
            if need_dx:
                dpatches = ops.gemm_nt(dy.view(m, cout), w2t)
                dx = torch.empty((n, d, h, w, cip), dtype=BF16, device=dev)
                call("mi_col2im3d", ptr(dpatches), ptr(dx), cip, n, d, h, w, cip, k, s, p)
                tape.put(x, _fit(dx, cin) if cip != cin else dx)

        tape.record(bwd)
    return y


def conv_transpose_gemm(ctx: E.Ctx, x, name, k, s, p, out_pad, relu):
    """nn.ConvTranspose3d(kernel k, stride s, padding p, output_padding out_pad) with bias (+ ReLU), weight `name.weight`
    [Cin, Cout, k, k, k], Cin % 8 == 0: the data gradient of the conv C (fine grid, Cout channels) -> (x's grid, Cin channels) that has
    the same weight tensor.  forward = fold(x . W2), input gradient = C's forward on dy, weight gradient = C's with (dy, x) in the
    roles of (input, output gradient)."""
    n, d, h, w, cin = x.shape
    wt = ctx.p(name + ".weight")
    cout, taps = wt.shape[1], k * k * k
    cop = _gemm_channels(cout, taps)
    fine = tuple((v - 1) * s - 2 * p + k + out_pad for v in (d, h, w))
    if any((f + 2 * p - k) // s + 1 != v for f, v in zip(fine, (d, h, w))) or min(fine) < 1:
        raise NotImplementedError(f"upsample_parameters: output_padding {out_pad} with stride {s} is not the data gradient of a conv")
    m, kk, dev = n * d * h * w, taps * cop, x.device
    nvox = n * fine[0] * fine[1] * fine[2]
    w2, w2t = _pack(wt, cin, cout, cop, taps)
    xd = ops.dense(x)
    dpatches = ops.gemm_nt(xd.view(m, cin), w2t)
    y0 = torch.empty((n,) + fine + (cop,), dtype=BF16, device=dev)
    call("mi_col2im3d", ptr(dpatches), ptr(y0), cop, n, *fine, cop, k, s, p)
    del dpatches
    y = torch.empty((n,) + fine + (cout,), dtype=BF16, device=dev)
    call("mi_bias_act_bf16", ptr(y0), cop, ptr(ctx.p(name + ".bias")), ptr(y), cout, nvox, cout, int(relu))
    del y0
    ctx.count(2 * m * cin * taps * cout)
    if ctx.tape is not None:
        tape = ctx.tape

        def bwd():
            dy = tape.take(y)
            if dy is None:
                return
            dy = ops.dense(dy)
            if relu:  # relu'(u) = [y > 0]
                g = torch.empty_like(dy)
                call("mi_leaky_relu_bwd", ptr(y), ptr(dy), ptr(g), dy.numel(), 0.0)
                dy = g
            _bias_grad(ctx, name, dy)
            dys = _fit(dy, cop) if cop != cout else dy
            patches = torch.empty((m, kk), dtype=BF16, device=dev)
            call("mi_im2col3d", ptr(dys), cop, ptr(patches), n, *fine, cop, k, s, p)
            _unpack_wgrad(E.token_wgrad(xd.view(m, cin), patches), ctx.g(name + ".weight"), cin, cout, cop, taps)
            tape.put(x, ops.gemm_nt(patches, w2).view(n, d, h, w, cin))

        tape.record(bwd)
    return y


# ------------------------------------------------------------------------------------------------ module
class _Quantize(torch.autograd.Function):
    """The `quantize` edge: z fp32 NCDHW -> (straight-through q fp32 NCDHW, loss); backward dz = dq + dloss * 2 cc (z - q) / numel."""

    @staticmethod
    def forward(ctx, module, z):
        z_cl = ops.to_channels_last(z.contiguous().float())
        zq, diff, loss, _ = module._quantize_cl(z_cl)
        ctx.diff, ctx.scale, ctx.shape = diff, 2.0 * module.commitment_cost / z_cl.numel(), z_cl.shape
        ctx.set_materialize_grads(False)
        return ops.to_channels_first(zq), loss.view(())

    @staticmethod
    def backward(ctx, dq, dloss):
        dev = ctx.diff.device
        weight = torch.zeros(1, dtype=F32, device=dev) if dloss is None else dloss.detach().float().reshape(1).contiguous()
        dq_cl = torch.zeros(ctx.shape, dtype=BF16, device=dev) if dq is None else ops.to_channels_last(dq.contiguous().float())
        return None, ops.to_channels_first(vq_bwd(dq_cl, ctx.diff, weight, ctx.scale))


class VQVAE(HipModule):
    """`generative.networks.nets.VQVAE(spatial_dims, in_channels, out_channels, num_channels, num_res_layers, num_res_channels,
    downsample_parameters=(stride, kernel, dilation, padding) per level, upsample_parameters=(stride, kernel, dilation, padding,
    output_padding) per level, num_embeddings, embedding_dim, embedding_init, commitment_cost, decay, epsilon, dropout, act, output_act,
    ddp_sync, use_checkpointing)`.  On the HIP path: spatial_dims 3, dilation 1, dropout 0, ReLU, no output activation, cubic kernels,
    channel counts in multiples of 8, embedding_dim <= 256, num_embeddings <= 8192; anything else raises NotImplementedError naming the
    keyword.  `train()` / `eval()` switch the EMA codebook update; the codebook and its EMA buffers are no optimizer state."""

    def __init__(self, spatial_dims: int, in_channels: int, out_channels: int, num_channels=(96, 96, 192), num_res_layers: int = 3,
                 num_res_channels=(96, 96, 192), downsample_parameters=((2, 4, 1, 1), (2, 4, 1, 1), (2, 4, 1, 1)),
                 upsample_parameters=((2, 4, 1, 1, 0), (2, 4, 1, 1, 0), (2, 4, 1, 1, 0)), num_embeddings: int = 32, embedding_dim: int = 64,
                 embedding_init: str = "normal", commitment_cost: float = 0.25, decay: float = 0.5, epsilon: float = 1e-5,
                 dropout: float = 0.0, act="RELU", output_act=None, ddp_sync: bool = True, use_checkpointing: bool = False) -> None:
        super().__init__()
        num_channels = tuple(num_channels)
        if isinstance(num_res_channels, int):
            num_res_channels = (num_res_channels,) * len(num_channels)
        num_res_channels = tuple(num_res_channels)
        if len(num_res_channels) != len(num_channels):
            raise ValueError("`num_res_channels` should be a single integer or a tuple of integers with the same length as `num_channels`.")
        ds, us = [tuple(t) for t in downsample_parameters], [tuple(t) for t in upsample_parameters]
        if len(ds) != len(num_channels):
            raise ValueError("`downsample_parameters` should be a tuple of tuples with the same length as `num_channels`.")
        if len(us) != len(num_channels):
            raise ValueError("`upsample_parameters` should be a tuple of tuples with the same length as `num_channels`.")
        if any(len(t) != 4 for t in ds):
            raise ValueError("`downsample_parameters` should be a tuple of tuples with 4 integers (stride, kernel, dilation, padding).")
        if any(len(t) != 5 for t in us):
            raise ValueError("`upsample_parameters` should be a tuple of tuples with 5 integers (stride, kernel, dilation, padding, "
                             "output_padding).")
        if spatial_dims != 3:
            raise NotImplementedError("spatial_dims: the HIP VQVAE is 3-D only")
        if any(t[2] != 1 for t in ds):
            raise NotImplementedError("downsample_parameters: dilation must be 1")
        if any(t[2] != 1 for t in us):
            raise NotImplementedError("upsample_parameters: dilation must be 1")
        if dropout:
            raise NotImplementedError("dropout > 0 is not on the HIP path")
        act_name = act[0] if isinstance(act, (tuple, list)) else act
        if str(act_name).upper() != "RELU":
            raise NotImplementedError("act: only ReLU")
        if output_act is not None:
            raise NotImplementedError("output_act is not on the HIP path")
        if any(not isinstance(v, int) for t in ds + us for v in t):
            raise NotImplementedError("downsample_parameters / upsample_parameters: cubic kernels only (one integer per field)")
        if any(c % 8 for c in num_channels + num_res_channels):
            raise NotImplementedError("num_channels / num_res_channels: multiples of 8 on the HIP path")
        if not 1 <= embedding_dim <= MAX_D:
            raise NotImplementedError(f"embedding_dim: 1 .. {MAX_D}")
        if not 1 <= num_embeddings <= MAX_K:
            raise NotImplementedError(f"num_embeddings: 1 .. {MAX_K}")
        if embedding_init not in ("normal", "kaiming_uniform"):
            raise ValueError("embedding_init: 'normal' or 'kaiming_uniform'")
        for (st, k, _, p, op) in us:
            if op >= st and not (op == 0 and st == 1):
                raise NotImplementedError(f"upsample_parameters: output_padding {op} with stride {st} is not the data gradient of a conv")

        self.spatial_dims, self.in_channels, self.out_channels = spatial_dims, in_channels, out_channels
        self.num_channels, self.num_res_layers, self.num_res_channels = num_channels, num_res_layers, num_res_channels
        self.num_embeddings, self.embedding_dim = num_embeddings, embedding_dim
        self.commitment_cost, self.decay, self.epsilon = float(commitment_cost), float(decay), float(epsilon)
        self.ddp_sync, self.use_checkpointing = bool(ddp_sync), bool(use_checkpointing)
        self.latent_channels = embedding_dim
        spec = ParamSpec(self, 3)
        L = len(num_channels)
        self._enc, self._dec = [], []

        def add(plan, prefix, kind, *args):
            name = f"{prefix}.blocks.{len(plan)}"
            plan.append((kind, name) + args)
            return name

        def res(plan, prefix, c, r):
            n = add(plan, prefix, "res")
            spec.conv(n + ".conv1.conv", c, r, 3)
            spec.conv(n + ".conv2.conv", r, c, 3)

        Ep = self._enc
        for i in range(L):
            st, k, _, p = ds[i]
            n = add(Ep, "encoder", "conv", k, st, p, True)  # monai Convolution: the conv and its ReLU are one block
            spec.conv(n + ".conv", in_channels if i == 0 else num_channels[i - 1], num_channels[i], k)
            for _ in range(num_res_layers):
                res(Ep, "encoder", num_channels[i], num_res_channels[i])
        spec.conv(add(Ep, "encoder", "conv", 3, 1, 1, False) + ".conv", num_channels[-1], embedding_dim, 3)

        Dp = self._dec
        rch, rrc = num_channels[::-1], num_res_channels[::-1]
        spec.conv(add(Dp, "decoder", "conv", 3, 1, 1, False) + ".conv", embedding_dim, rch[0], 3)
        for i in range(L):
            for _ in range(num_res_layers):
                res(Dp, "decoder", rch[i], rrc[i])
            st, k, _, p, op = us[i]
            cout = out_channels if i == L - 1 else rch[i + 1]
            n = add(Dp, "decoder", "convT", k, st, p, op, i != L - 1)
            wt, b = torch.empty(rch[i], cout, k, k, k), torch.empty(cout)  # nn.ConvTranspose3d: weight [in, out, k, k, k]
            nn.init.kaiming_uniform_(wt, a=5 ** 0.5)
            bound = 1 / (cout * k ** 3) ** 0.5  # torch takes fan_in from dim 1 of the weight
            spec._add(n + ".conv.weight", wt)
            spec._add(n + ".conv.bias", b.uniform_(-bound, bound))

        self._init_plumbing(spec, [])
        # quantizer.quantizer.*: outside the arena (no optimizer state, no clip norm)
        e = torch.empty(num_embeddings, embedding_dim)
        if embedding_init == "kaiming_uniform":
            nn.init.kaiming_uniform_(e, mode="fan_in", nonlinearity="linear")
        else:
            nn.init.normal_(e)
        q = nn.Module()
        q.embedding = nn.Module()
        q.embedding.register_parameter("weight", nn.Parameter(e, requires_grad=False))
        q.register_buffer("ema_cluster_size", torch.ones(num_embeddings))
        q.register_buffer("ema_w", e.clone())
        self.quantizer = nn.Module()
        self.quantizer.quantizer = q
        self.quantizer.perplexity = torch.zeros(1)
        self.encoder.spatial_dims, self.encoder.in_channels = spatial_dims, in_channels

    # ------------------------------------------------------------------------------------------ engine
    @property
    def codebook(self):
        return self.quantizer.quantizer.embedding.weight

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self.quantizer.perplexity = fn(self.quantizer.perplexity)
        return out

    def _run_plan(self, c: E.Ctx, plan, x, need_dx):
        if self.use_checkpointing and c.tape is not None:
            return E.checkpoint(c, lambda cc, xx: self._run_plan_body(cc, plan, xx, need_dx), x)
        return self._run_plan_body(c, plan, x, need_dx)

    def _run_plan_body(self, c: E.Ctx, plan, x, need_dx):
        first = True
        for step in plan:
            kind, name = step[0], step[1]
            ndx = need_dx or not first
            if kind == "conv":
                k, s, p = step[2:5]
                if (k, s, p) == (3, 1, 1):
                    x = conv_k3(c, x, name + ".conv", need_dx=ndx)
                else:
                    x = conv_gemm(c, x, name + ".conv", k, s, p, need_dx=ndx)
                if step[5]:
                    x = leaky_relu(c, x, 0.0)
            elif kind == "res":  # relu(x + conv2(relu(conv1(x))))
                h = leaky_relu(c, conv_k3(c, x, name + ".conv1.conv"), 0.0)
                x = leaky_relu(c, conv_k3(c, h, name + ".conv2.conv", res=x), 0.0)
            elif kind == "convT":
                x = conv_transpose_gemm(c, x, name + ".conv", *step[2:7])
            first = False
        return x

    def _quantize_cl(self, z_cl, update=None, loss=None):
        """z_cl bf16 NDHWC -> (zq, diff, loss [1], idx int32); the EMA update (training mode, or `update`) runs AFTER q was gathered.
        loss: the fp32 [1] device scalar to write the quantization loss into."""
        q = self.quantizer.quantizer
        cb = q.embedding.weight.data
        idx = vq_assign(z_cl, cb)
        zq, diff, loss = vq_gather_loss(z_cl, cb, idx, self.commitment_cost, loss)
        if self.training if update is None else update:
            if self.ddp_sync and torch.distributed.is_available() and torch.distributed.is_initialized() and \
                    torch.distributed.get_world_size() > 1:
                raise NotImplementedError("ddp_sync: the all-reduce of the codebook statistics over a process group is not on the HIP path")
            vq_ema_update(z_cl, idx, cb, q.ema_cluster_size, q.ema_w, self.decay, self.epsilon, self.quantizer.perplexity)
        return zq, diff, loss, idx

    # ------------------------------------------------------------------------------------------ upstream API
    def _check(self, x, channels):
        if not x.is_cuda:
            raise RuntimeError("medical_image_generation_amd runs on MI355X only: move the module and inputs to 'cuda' "
                               "(there is no CPU fallback; the CPU restatement lives in tests/vqvae_ref.py)")
        if x.dim() != 5 or x.shape[1] != channels:
            raise ValueError(f"expected [N, {channels}, D, H, W], got {tuple(x.shape)}")

    def _edge(self, runner, x):
        grad_enabled = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        return _NetFn.apply(self, runner, 1, grad_enabled, x, None, *self.parameters())

    def encode(self, images):
        self._check(images, self.in_channels)

        def runner(c, xin, need_dx):
            x_cl = ops.to_channels_last(xin.contiguous().float())
            return (self._run_plan(c, self._enc, x_cl, need_dx),), {"x_cl": x_cl}

        return self._edge(runner, images)

    def quantize(self, encodings):
        self._check(encodings, self.embedding_dim)
        q, loss = _Quantize.apply(self, encodings)
        return q, loss

    def decode(self, quantizations):
        self._check(quantizations, self.embedding_dim)

        def runner(c, zin, need_dx):
            z_cl = ops.to_channels_last(zin.contiguous().float())
            return (self._run_plan(c, self._dec, z_cl, need_dx),), {"x_cl": z_cl}

        return self._edge(runner, quantizations)

    def index_quantize(self, images):
        z = self.encode(images)
        with torch.no_grad():
            return vq_assign(ops.to_channels_last(z.detach()), self.codebook.data).long()

    def decode_samples(self, embedding_indices):
        if not embedding_indices.is_cuda:
            raise RuntimeError("medical_image_generation_amd runs on MI355X only (no CPU fallback)")
        idx = embedding_indices.to(I32).contiguous()
        return self.decode(ops.to_channels_first(vq_embed(idx, self.codebook.data)))

    def forward(self, images):
        quantizations, quantization_losses = self.quantize(self.encode(images))
        return self.decode(quantizations), quantization_losses

    def encode_stage_2_inputs(self, x):
        return self.encode(x)

    def decode_stage_2_outputs(self, z):
        e, _ = self.quantize(z)
        return self.decode(e)
