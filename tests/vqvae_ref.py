"""Torch restatement of MONAI-Generative 0.2.x `VQVAE` / `EMAQuantizer` (third-party; not installed, not under the reference tree:
PARITY UNPINNED) -- the arithmetic the issue's section "What upstream computes" fixes, in fp32 or fp64, for the tests only.

Everything behind the argmin is discontinuous in the index, and a bf16 encoder legitimately picks another code than an fp32 one for a
token near a tie.  So the quantiser takes `forced_idx`: the tests compare the encoder output, then the indices given the device's own
z, then the decoder and every gradient given the device's indices."""
import math

import torch
from torch import nn


def nearest_code(x, e):
    """argmin_k |x_t - e_k|^2 over rows, in the dtype of the inputs; ties to the lowest index (torch.argmin is not pinned: min of
    the indices that attain the minimum)."""
    d = (x * x).sum(1, keepdim=True) - 2 * x @ e.t() + (e * e).sum(1)[None]
    m = d.min(1, keepdim=True).values
    k = torch.arange(e.shape[0])[None].expand_as(d)
    return torch.where(d == m, k, torch.full_like(k, e.shape[0])).min(1).values


def ema_update(x, idx, emb, cluster, ema_w, decay, eps):
    """One training-mode update (tensors of one dtype): -> embedding, ema_cluster_size, ema_w, perplexity, counts, dw."""
    K, T = emb.shape[0], x.shape[0]
    counts = torch.bincount(idx, minlength=K).to(x.dtype)
    cluster = decay * cluster + (1 - decay) * counts
    n = cluster.sum()
    w = (cluster + eps) / (n + K * eps) * n
    dw = torch.zeros_like(ema_w).index_add_(0, idx, x)
    ema_w = decay * ema_w + (1 - decay) * dw
    p = counts / T
    return ema_w / w[:, None], cluster, ema_w, torch.exp(-(p * torch.log(p + 1e-10)).sum()), counts, dw


class Quantizer(nn.Module):
    def __init__(self, num_embeddings, embedding_dim, commitment_cost=0.25, decay=0.5, epsilon=1e-5, embedding_init="normal", dtype=torch.float32):
        super().__init__()
        w = torch.empty(num_embeddings, embedding_dim, dtype=dtype)
        if embedding_init == "kaiming_uniform":
            nn.init.kaiming_uniform_(w, mode="fan_in", nonlinearity="linear")
        else:
            nn.init.normal_(w)
        self.embedding = nn.Embedding(num_embeddings, embedding_dim, _weight=w)
        self.embedding.weight.requires_grad = False
        self.register_buffer("ema_cluster_size", torch.ones(num_embeddings, dtype=dtype))
        self.register_buffer("ema_w", w.clone())
        self.commitment_cost, self.decay, self.epsilon = commitment_cost, decay, epsilon
        self.perplexity = None

    def forward(self, z, forced_idx=None):
        """z [N, C, D, H, W] -> (loss, straight-through output, idx [N, D, H, W])."""
        dt = self.embedding.weight.dtype
        zl = z.to(dt).permute(0, 2, 3, 4, 1).contiguous()
        flat = zl.reshape(-1, zl.shape[-1])
        idx = nearest_code(flat.detach(), self.embedding.weight) if forced_idx is None else forced_idx.reshape(-1).long()
        q = self.embedding.weight[idx].view(zl.shape)  # gathered from the OLD codebook
        if self.training:
            with torch.no_grad():
                e, c, w, self.perplexity, _, _ = ema_update(flat.detach(), idx, self.embedding.weight, self.ema_cluster_size, self.ema_w,
                                                            self.decay, self.epsilon)
                q = q.clone()
                self.embedding.weight.copy_(e), self.ema_cluster_size.copy_(c), self.ema_w.copy_(w)
        loss = self.commitment_cost * torch.mean((q.detach() - zl) ** 2)
        out = zl + (q - zl).detach()
        return loss, out.permute(0, 4, 1, 2, 3).contiguous(), idx.view(zl.shape[:-1])


class _Wrap(nn.Module):  # monai's Convolution: `.conv.weight` names, the activation inside the same block
    def __init__(self, conv, relu=False):
        super().__init__()
        self.conv, self.relu = conv, relu

    def forward(self, x):
        return torch.relu(self.conv(x)) if self.relu else self.conv(x)


class _Res(nn.Module):
    def __init__(self, c, r):
        super().__init__()
        self.conv1, self.conv2 = _Wrap(nn.Conv3d(c, r, 3, padding=1)), _Wrap(nn.Conv3d(r, c, 3, padding=1))

    def forward(self, x):
        return torch.relu(x + self.conv2(torch.relu(self.conv1(x))))


class _Seq(nn.Module):
    def __init__(self, blocks):
        super().__init__()
        self.blocks = nn.ModuleList(blocks)

    def forward(self, x):
        for b in self.blocks:
            x = b(x)
        return x


class _QWrap(nn.Module):  # `quantizer.quantizer.*`
    def __init__(self, q):
        super().__init__()
        self.quantizer = q


def check_arguments(num_channels, num_res_channels, downsample_parameters, upsample_parameters):
    if isinstance(num_res_channels, int):
        num_res_channels = (num_res_channels,) * len(num_channels)
    if len(num_res_channels) != len(num_channels):
        raise ValueError("`num_res_channels` should be a single integer or a tuple of integers with the same length as `num_channels`.")
    if len(downsample_parameters) != len(num_channels) or len(upsample_parameters) != len(num_channels):
        raise ValueError("`downsample_parameters` and `upsample_parameters` should have one tuple per level of `num_channels`.")
    if any(len(t) != 4 for t in downsample_parameters):
        raise ValueError("`downsample_parameters` should be tuples of (stride, kernel, dilation, padding).")
    if any(len(t) != 5 for t in upsample_parameters):
        raise ValueError("`upsample_parameters` should be tuples of (stride, kernel, dilation, padding, output_padding).")
    return tuple(num_res_channels)


class VQVAE(nn.Module):
    def __init__(self, spatial_dims, in_channels, out_channels, num_channels=(96, 96, 192), num_res_layers=3, num_res_channels=(96, 96, 192),
                 downsample_parameters=((2, 4, 1, 1),) * 3, upsample_parameters=((2, 4, 1, 1, 0),) * 3, num_embeddings=32, embedding_dim=64,
                 embedding_init="normal", commitment_cost=0.25, decay=0.5, epsilon=1e-5, dropout=0.0, act="RELU", output_act=None,
                 ddp_sync=True, use_checkpointing=False, dtype=torch.float32):
        super().__init__()
        assert spatial_dims == 3
        nrc = check_arguments(num_channels, num_res_channels, downsample_parameters, upsample_parameters)
        L = len(num_channels)
        enc = []
        for i in range(L):
            s, k, _, p = downsample_parameters[i]
            enc.append(_Wrap(nn.Conv3d(in_channels if i == 0 else num_channels[i - 1], num_channels[i], k, s, p), relu=True))
            enc += [_Res(num_channels[i], nrc[i]) for _ in range(num_res_layers)]
        enc.append(_Wrap(nn.Conv3d(num_channels[-1], embedding_dim, 3, padding=1)))
        dec = [_Wrap(nn.Conv3d(embedding_dim, num_channels[-1], 3, padding=1))]
        rch, rrc = list(reversed(num_channels)), list(reversed(nrc))
        for i in range(L):
            dec += [_Res(rch[i], rrc[i]) for _ in range(num_res_layers)]
            s, k, _, p, op = upsample_parameters[i]
            dec.append(_Wrap(nn.ConvTranspose3d(rch[i], out_channels if i == L - 1 else rch[i + 1], k, s, p, output_padding=op), relu=i != L - 1))
        self.encoder, self.decoder = _Seq(enc), _Seq(dec)
        self.quantizer = _QWrap(Quantizer(num_embeddings, embedding_dim, commitment_cost, decay, epsilon, embedding_init, dtype))
        self.to(dtype)
        self.dtype_ = dtype

    def encode(self, x):
        return self.encoder(x.to(self.dtype_))

    def quantize(self, z, forced_idx=None):
        loss, q, _ = self.quantizer.quantizer(z, forced_idx)
        return q, loss

    def decode(self, q):
        return self.decoder(q.to(self.dtype_))

    def index_quantize(self, x):
        return self.quantizer.quantizer(self.encode(x))[2]

    def decode_samples(self, idx):
        e = self.quantizer.quantizer.embedding.weight[idx.long()]  # [N, D, H, W, C]
        return self.decode(e.permute(0, 4, 1, 2, 3).contiguous())

    def forward(self, x, forced_idx=None):
        q, loss = self.quantize(self.encode(x), forced_idx)
        return self.decode(q), loss


def seeded_tokens(T, D, K, seed=1):
    """The inputs of the assign tests: N(0, 1) tokens (rounded to bf16, as the kernel reads them) and N(0, 1) fp32 codes."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * T + 31 * D + K)
    x = torch.randn(T, D, generator=g).to(torch.bfloat16)
    e = torch.randn(K, D, generator=g)
    return x, e


def assign_tolerance(x, e):
    """tau_t = 16 * 2^-24 * (D + 2) * (|x_t| + max_k |e_k|)^2 (fp64): the fp32 rounding bound of the dot product and the norms."""
    x, e = x.double(), e.double()
    return 16 * 2.0 ** -24 * (x.shape[1] + 2) * (x.norm(dim=1) + e.norm(dim=1).max()) ** 2


def near_tie_share(x, e):
    """Share of tokens whose fp64 best / second-best distance gap is below tau (1 code: 0)."""
    if e.shape[0] < 2:
        return 0.0
    xd, ed = x.double(), e.double()
    d = (xd * xd).sum(1, keepdim=True) - 2 * xd @ ed.t() + (ed * ed).sum(1)[None]
    two = d.topk(2, dim=1, largest=False).values
    return float(((two[:, 1] - two[:, 0]) < assign_tolerance(x, e)).double().mean())


ASSIGN_SHAPES = [(1000, 3, 37), (513, 64, 32), (4096, 64, 512), (4099, 8, 2048), (64, 5, 1)]
