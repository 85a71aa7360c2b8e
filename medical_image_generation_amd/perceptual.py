"""LPIPS-VGG perceptual loss on the MI355X HIP path.

The reference's generator step adds `perceptual_loss(reconstructions.float(), images.float()) * perc_weight` (train_autoencoder.py:416,
perc_weight 0.125) with `PerceptualLoss(**perceptual_params)` built at train_autoencoder.py:601 from the planner's
`{'spatial_dims': 3, 'network_type': 'vgg', 'is_fake_3d': True, 'fake_3d_ratio': 0.2}` (2-D datasets: `{'spatial_dims': 2,
'network_type': 'vgg'}`, configuration.py:961-964).  The class comes from the third-party `generative` package (which wraps `lpips.LPIPS`
v0.1 in eval mode); its source is not part of the reference, so what follows is a restatement -- PARITY UNPINNED against upstream:

  LPIPS(x, y) = sum over the 5 VGG16 levels (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3) of
                mean over pixels of  sum_c w_c (f_x / (|f_x| + 1e-10) - f_y / (|f_y| + 1e-10))_c^2
  after the scaling layer (x - shift) / scale (a 1-channel input broadcasts to 3 channels).
  Fake 3-D (3-D inputs, is_fake_3d): for each spatial axis 2, 3, 4 (in that order) the volume is cut into N * extent 2-D slices
  (n-major; pixel axes = the other two spatial axes in order), int(N * extent * fake_3d_ratio) of them are picked by
  `torch.randperm` on the CPU generator, and the mean LPIPS of the picked slices is taken; the loss is the sum of the three means.
  2-D inputs: the mean LPIPS of the image batch.

The weights are an INPUT (`weights=`: a state_dict or a `.pth` path, produced once with upstream's own class -- INTEGRATION.md): the
pretrained VGG / lin weights cannot be downloaded here, and a perceptual loss with random weights is a wrong answer, so the constructor
refuses to build one unless `pretrained=False` is passed explicitly (tests).

Kernels (csrc/perceptual.hip + the library's 2-D conv plans): slice gather with the scaling layer -> 13 x (3x3 conv forward + ReLU,
fused with the 2x2 max-pool at the end of levels 1-4) on both branches level by level, the LPIPS head of each level as one pass (loss
and the gradient w.r.t. the reconstruction branch's feature; the target branch's features are dropped right after it) -> data
gradients back down the reconstruction branch (ReLU / max-pool backward fused, never a weight gradient: the network is frozen) ->
scatter-add into the gradient of the volume.
"""
from __future__ import annotations

import torch
from torch import nn

from . import hipops as ops
from ._lib import call, ptr

BF16, F32 = torch.bfloat16, torch.float32

# torchvision vgg16().features: (index, cin, cout) of the 3x3 convs, grouped by lpips' slices 1..5 (each slice ends with a ReLU whose
# output is the level's feature; slices 2..5 start with a 2x2 max-pool)
VGG_LEVELS = (
    ((0, 3, 64), (2, 64, 64)),
    ((5, 64, 128), (7, 128, 128)),
    ((10, 128, 256), (12, 256, 256), (14, 256, 256)),
    ((17, 256, 512), (19, 512, 512), (21, 512, 512)),
    ((24, 512, 512), (26, 512, 512), (28, 512, 512)),
)
_SLICE_END = (4, 9, 16, 23, 30)  # slice k holds features[_SLICE_END[k-1] : _SLICE_END[k]]
LPIPS_EPS = 1e-10
_SHIFT = (-0.030, -0.088, -0.188)
_SCALE = (0.458, 0.448, 0.450)


class _ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(_SHIFT, dtype=F32)[None, :, None, None])
        self.register_buffer("scale", torch.tensor(_SCALE, dtype=F32)[None, :, None, None])


class _VGG16Slices(nn.Module):
    """Parameter holder with lpips' `pn.vgg16` layout: slice1..slice5 = nn.Sequential of torchvision's feature indices (never called)."""

    def __init__(self):
        super().__init__()
        convs = {i: (cin, cout) for level in VGG_LEVELS for i, cin, cout in level}
        start = 0
        for k, end in enumerate(_SLICE_END, 1):
            seq = nn.Sequential()
            for i in range(start, end):
                if i in convs:
                    seq.add_module(str(i), nn.Conv2d(convs[i][0], convs[i][1], 3, padding=1))
                elif i - 1 in convs:
                    seq.add_module(str(i), nn.ReLU())
                else:
                    seq.add_module(str(i), nn.MaxPool2d(2, 2))
            setattr(self, f"slice{k}", seq)
            start = end


class _NetLinLayer(nn.Module):
    def __init__(self, chn_in):
        super().__init__()
        self.model = nn.Sequential(nn.Dropout(), nn.Conv2d(chn_in, 1, 1, stride=1, padding=0, bias=False))


class _LPIPS(nn.Module):
    def __init__(self):
        super().__init__()
        self.scaling_layer = _ScalingLayer()
        self.net = _VGG16Slices()
        for k, level in enumerate(VGG_LEVELS):
            setattr(self, f"lin{k}", _NetLinLayer(level[-1][2]))


def _he_init_(lp: _LPIPS):
    """Random weights for pretrained=False: He-normal convs (activations survive 13 layers), zero biases, non-negative heads."""
    for level in VGG_LEVELS:
        for i, cin, _ in level:
            conv = _conv(lp, i)
            nn.init.normal_(conv.weight, 0.0, (2.0 / (cin * 9)) ** 0.5)
            nn.init.zeros_(conv.bias)
    for k in range(len(VGG_LEVELS)):
        nn.init.uniform_(getattr(lp, f"lin{k}").model[1].weight, 0.0, 0.1)


def _conv(lp: _LPIPS, i: int) -> nn.Conv2d:
    k = next(k for k, end in enumerate(_SLICE_END, 1) if i < end)
    return getattr(lp.net, f"slice{k}")._modules[str(i)]


class PerceptualLoss(nn.Module):
    """`generative.losses.PerceptualLoss(spatial_dims, network_type="vgg", is_fake_3d=True, fake_3d_ratio=0.5, ...)` for
    network_type="vgg" (LPIPS v0.1).  `weights`: upstream's `PerceptualLoss(...).state_dict()` (or a `.pth` path of one); without it
    the constructor raises unless `pretrained=False` (random weights, tests).

    `forward(input, target[, indices])` works on torch tensors (fp32 NC[D]HW on the GPU) with an autograd edge for `input` only -- a
    drop-in for `AETrainer(extra_loss=...)` callers.  `hip(...)` is the fused form of the trainers on channels-last bf16 tensors."""

    def __init__(self, spatial_dims: int, network_type: str = "vgg", is_fake_3d: bool = True, fake_3d_ratio: float = 0.5,
                 cache_dir=None, pretrained: bool = True, pretrained_path=None, pretrained_state_dict_key=None, weights=None):
        super().__init__()
        if network_type != "vgg":
            raise NotImplementedError(f"network_type={network_type!r}: only 'vgg' (LPIPS-VGG) is on the HIP path")
        if spatial_dims not in (2, 3):
            raise NotImplementedError("Perceptual loss is implemented only in 2D and 3D.")
        if spatial_dims == 3 and not is_fake_3d:
            raise NotImplementedError("3-D LPIPS-VGG runs as fake 3-D (is_fake_3d=True), as upstream does")
        if not 0.0 <= fake_3d_ratio <= 1.0:
            raise ValueError("fake_3d_ratio must be in [0, 1]")
        self.spatial_dims, self.network_type = spatial_dims, network_type
        self.is_fake_3d, self.fake_3d_ratio = is_fake_3d, float(fake_3d_ratio)
        self.perceptual_function = _LPIPS()
        if weights is None and pretrained_path is not None:
            weights = pretrained_path
        if weights is not None:
            self.load_weights(weights)
        elif pretrained:
            raise ValueError("PerceptualLoss(network_type='vgg') needs the pretrained LPIPS-VGG weights: pass weights=<upstream "
                             "PerceptualLoss(...).state_dict() or a .pth path of one> (INTEGRATION.md), or pretrained=False for random "
                             "weights (tests only)")
        else:
            _he_init_(self.perceptual_function)
        for p in self.parameters():
            p.requires_grad_(False)  # frozen, like upstream
        self.eval()
        self._plans = {}
        self._w1 = None      # conv1_1's weight zero-padded to 8 input channels
        self._arange = {}    # (device, N) -> int32 arange: the slice list of a 2-D batch

    # ------------------------------------------------------------------ weights
    def load_weights(self, weights):
        """Load upstream's state_dict (or a path of one).  `perceptual_function.lins.k.*` (lpips registers its heads twice: as lin<k> and
        in the ModuleList `lins`) are the same tensors as `lin<k>.*` and are dropped."""
        if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__"):
            weights = torch.load(weights, map_location="cpu", weights_only=True)
        sd = {k: v for k, v in weights.items() if not k.startswith("perceptual_function.lins.")}
        self.load_state_dict(sd, strict=True)

    # ------------------------------------------------------------------ slice selection (upstream's randperm draws)
    def draw_indices(self, shape, generator=None):
        """The slice indices upstream's fake-3D forward draws for an input of `shape` (N, C, D, H, W): one
        `torch.randperm(N * extent, generator=generator)[:int(N * extent * fake_3d_ratio)]` per spatial axis 2, 3, 4, in that order
        (CPU int64).  [] for 2-D inputs (no draw)."""
        if len(shape) != 5 or not (self.spatial_dims == 3 and self.is_fake_3d):
            return []
        out = []
        for axis in (2, 3, 4):
            s = shape[0] * shape[axis]
            out.append(torch.randperm(s, generator=generator)[: int(s * self.fake_3d_ratio)])
        return out

    # ------------------------------------------------------------------ fused form
    def _plan(self, i, cin, cout, s, a, b):
        key = (i, s, a, b)  # one plan per conv: a plan holds ONE packed weight (layers of equal shape must not share it)
        p = self._plans.get(key)
        if p is None:
            p = self._plans[key] = ops.ConvPlan(s, (1, a, b), cin, cout, (1, 3, 3), (1, 1, 1), (0, 1, 1))
        return p

    def _weight(self, i):
        conv = _conv(self.perceptual_function, i)
        if i == 0:
            if self._w1 is None or self._w1.device != conv.weight.device:
                self._w1 = torch.empty((64, 8, 3, 3), dtype=F32, device=conv.weight.device)
            call("mi_pad_cin_f32", ptr(conv.weight), ptr(self._w1), 64, 3, 8, 9)
            return self._w1, conv.bias
        return conv.weight, conv.bias

    def _check_device(self, x):
        sl = self.perceptual_function.scaling_layer
        if not x.is_cuda or sl.shift.device != x.device:
            raise RuntimeError("PerceptualLoss runs on MI355X only: move the module and the inputs to the same 'cuda' device")

    def slice_lists(self, x_cl, indices):
        """[(axis, int32 device indices)] for a channels-last input: the 3 fake-3D axes, or the whole batch of a 2-D input."""
        n, d = x_cl.shape[0], x_cl.shape[1]
        if self.spatial_dims == 2 or d == 1:
            key = (x_cl.device, n)
            if key not in self._arange:
                self._arange[key] = torch.arange(n, dtype=torch.int32, device=x_cl.device)
            return [(0, self._arange[key])]
        if indices is None or len(indices) != 3:
            raise ValueError("fake 3-D needs three index tensors (draw_indices)")
        out = []
        for axis, idx in enumerate(indices):
            if not idx.is_cuda or idx.dtype != torch.int32 or idx.dim() != 1 or not idx.is_contiguous() or idx.numel() == 0:
                raise ValueError("slice indices must be non-empty contiguous int32 device vectors")
            out.append((axis, idx))
        return out

    def hip(self, x_cl, target_cl, indices, loss_acc, weight: float, grad=None, want_grad=True):
        """Fused form on channels-last bf16 [N, D, H, W, C] tensors (2-D: D = 1), C in {1, 3}: *loss_acc += weight * loss.
        indices: three int32 device vectors (fake 3-D; ignored for 2-D).  The gradient d(weight * loss)/d(x) is ADDED into `grad`
        (channels-last bf16 like x) when given, else returned in a fresh zeroed tensor; want_grad=False: forward only (returns None)."""
        self._check_device(x_cl)
        if x_cl.dtype != BF16 or target_cl.dtype != BF16 or x_cl.shape != target_cl.shape or x_cl.dim() != 5:
            raise ValueError("x and target must be channels-last bf16 tensors of one shape [N, D, H, W, C]")
        n, d, h, w, c = x_cl.shape
        if c not in (1, 3):
            raise ValueError(f"LPIPS takes 1- or 3-channel images, got {c} channels")
        if want_grad and grad is None:
            grad = torch.zeros_like(x_cl)
        packed = set()
        for axis, idx in self.slice_lists(x_cl, indices):
            self._axis(x_cl, target_cl, axis, idx, loss_acc, float(weight), grad if want_grad else None, packed)
        return grad if want_grad else None

    def _axis(self, x_cl, t_cl, axis, idx, loss_acc, weight, grad, packed):
        lp = self.perceptual_function
        sl = lp.scaling_layer
        n, d, h, w, c = x_cl.shape
        s = idx.numel()
        a, b = (h, w) if axis == 0 else ((d, w) if axis == 1 else (d, h))
        xs = torch.empty((s, 1, a, b, 8), dtype=BF16, device=x_cl.device)
        ts = torch.empty_like(xs)
        for src, dst in ((x_cl, xs), (t_cl, ts)):
            call("mi_perc_gather", ptr(src), ops._cs(src), c, n, d, h, w, axis, ptr(idx), s, ptr(sl.shift), ptr(sl.scale), ptr(dst))
        saved = []
        hx, ht = xs, ts
        for k, level in enumerate(VGG_LEVELS):
            ins, plans = [], []
            for j, (i, cin, cout) in enumerate(level):
                cin = 8 if i == 0 else cin
                plan = self._plan(i, cin, cout, s, hx.shape[2], hx.shape[3])
                wt, bias = self._weight(i)
                if id(plan) not in packed:  # (the three axes of a cube share their plans: packed once per call)
                    plan.pack(wt)
                    packed.add(id(plan))
                zx, zt = plan.fwd(hx, addvec=bias), plan.fwd(ht, addvec=bias)
                pool = j == len(level) - 1 and k < len(VGG_LEVELS) - 1
                px = pt = None
                if pool:
                    po = (s, 1, zx.shape[2] // 2, zx.shape[3] // 2, cout)
                    px, pt = torch.empty(po, dtype=BF16, device=zx.device), torch.empty(po, dtype=BF16, device=zx.device)
                for z, p in ((zx, px), (zt, pt)):
                    call("mi_relu_maxpool2_fwd", ptr(z), ptr(p), s, z.shape[2], z.shape[3], cout)
                if grad is not None:
                    ins.append(hx)
                    plans.append(plan)
                hx, ht = zx, zt
            cout = level[-1][2]
            dhead = torch.empty_like(hx) if grad is not None else None
            call("mi_lpips_head", ptr(hx), ptr(ht), ptr(getattr(lp, f"lin{k}").model[1].weight), s, hx.shape[2] * hx.shape[3], cout,
                 weight, LPIPS_EPS, ptr(loss_acc), ptr(dhead))
            if grad is not None:
                saved.append((ins, plans, hx, dhead))
            if px is not None:
                hx, ht = px, pt  # (the target branch's feature of this level is released here)
        if grad is None:
            return
        dp = None
        while saved:
            ins, plans, feat, dhead = saved.pop()
            _, _, fh, fw, fc = feat.shape
            call("mi_relu_maxpool2_bwd", ptr(feat), ptr(dp), ptr(dhead), ptr(dhead), s, fh, fw, fc)  # in place: dhead -> d(pre-ReLU)
            dz = dhead
            for j in range(len(plans) - 1, -1, -1):
                dh = plans[j].dgrad(dz)
                if j > 0:
                    x_in = ins[j]  # the ReLU output that fed conv j: its mask
                    call("mi_relu_maxpool2_bwd", ptr(x_in), None, ptr(dh), ptr(dh), s, x_in.shape[2], x_in.shape[3], x_in.shape[4])
                    dz = dh
                else:
                    dp = dh
        call("mi_perc_scatter_add", ptr(dp), axis, ptr(idx), s, n, d, h, w, c, ptr(sl.scale), ptr(grad), ops._cs(grad))

    # ------------------------------------------------------------------ torch form
    def forward(self, input: torch.Tensor, target: torch.Tensor, indices=None):
        """Scalar loss (upstream's `torch.mean(loss)`); the gradient flows to `input` only.  indices: the three CPU or device index
        tensors of a fake-3D call (default: drawn here with draw_indices, as upstream draws inside its forward)."""
        if input.shape != target.shape:
            raise ValueError(f"ground truth has differing shape ({target.shape}) from input ({input.shape})")
        if input.dim() != self.spatial_dims + 2:
            raise ValueError(f"expected a {self.spatial_dims}-D batch, got shape {tuple(input.shape)}")
        self._check_device(input)
        if self.spatial_dims == 3:
            if indices is None:
                indices = self.draw_indices(tuple(input.shape))
            indices = [i.to(device=input.device, dtype=torch.int32).contiguous() for i in indices]
        return _PerceptualFn.apply(self, input, target, indices)


class _PerceptualFn(torch.autograd.Function):
    @staticmethod
    def forward(fctx, mod, x, target, indices):
        x_cl = ops.to_channels_last(x.detach().float())
        t_cl = ops.to_channels_last(target.detach().float())
        loss = torch.zeros(1, dtype=F32, device=x.device)
        g = mod.hip(x_cl, t_cl, indices, loss, 1.0, want_grad=fctx.needs_input_grad[1])
        fctx.g_cl, fctx.sd, fctx.xdtype = g, x.dim() - 2, x.dtype
        return loss.reshape(())

    @staticmethod
    def backward(fctx, gout):
        g = ops.to_channels_first(fctx.g_cl, fctx.sd) * gout
        fctx.g_cl = None
        return None, g.to(fctx.xdtype), None, None
