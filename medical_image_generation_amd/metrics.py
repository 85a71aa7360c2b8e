"""SSIM / MS-SSIM with batched pairwise scoring, and FID / MMD / KID, on the MI355X HIP path.

The LDM's validation (train_ldm.py:266-330, `LDM.validate_main`) scores the diversity of its samples with
`MultiScaleSSIMMetric(spatial_dims, data_range=1.0, kernel_size=4)` and `SSIMMetric(...)` with the same arguments (:276-277), one call
per unordered pair of the sampled images (:315-321).  Both classes come from the third-party `generative.metrics` package (monai's
metric conventions); its source is not part of the reference, so what follows is a restatement -- PARITY UNPINNED against upstream:

  per axis i:  gaussian: t = arange((1-k_i)/2, (1+k_i)/2, 1),  g_i = exp(-(t/sigma_i)^2 / 2) / sum(...)   (k = 4: taps at +-0.5, +-1.5)
               uniform:  g_i = 1/k_i
  G = outer product of g_0 .. g_{sd-1} (axis 0 = D for 3-D, H for 2-D), per channel, VALID (no padding)
  mu_x = G*x, mu_y = G*y, s_x = G*(x*x) - mu_x^2, s_y = G*(y*y) - mu_y^2, s_xy = G*(x*y) - mu_x*mu_y
  c1 = (k1*L)^2, c2 = (k2*L)^2, L = data_range
  cs = (2 s_xy + c2) / (s_x + s_y + c2),  ssim = ((2 mu_x mu_y + c1) / (mu_x^2 + mu_y^2 + c1)) * cs
  SSIM(b) = mean over channels and valid voxels of ssim
  MS-SSIM(b): for s in 0..S-1: m_s = relu(mean cs at scale s), then x, y = avg_pool(2, stride 2, floor) per spatial axis;
              m_{S-1} is replaced by relu(mean ssim at scale S-1);  MS-SSIM = prod_s m_s ** w_s
  size rule (MS-SSIM): extent_i // max(1, S-1)**2 must be > k_i - 1 on every axis (upstream's check, as is)

`pairwise(images, *metrics)` is the drop-in for the loop at train_ldm.py:315-321: one launch per scale scores every pair, each image's
pyramid is built once, and an `SSIMMetric` that shares kernel, constants and data range with a `MultiScaleSSIMMetric` reads the
latter's scale-0 sums.

Kernels (csrc/metrics.hip): a fused pair kernel per scale (the window's means, variances and covariance merged along W and H in LDS,
along D in registers, by a running-mean / running-spread update in which flat regions have exactly zero variance; ssim / cs
summed per output tile: no per-voxel map reaches HBM), the 2x average pool of the pyramid, and a per-pair finalize in fp64 in a fixed
order.  The tiling depends only on the shape and the kernel, so results are bit for bit reproducible and `pairwise` equals the
per-pair `__call__` exactly.  Torch only allocates (and casts non-fp32 inputs once).

Distribution metrics (train_ldm.py:32 imports `FIDMetric, MMDMetric`; :308-310 `fid(synth_features, real_features)`).  They take
feature matrices, as upstream's do: the feature networks (RadImageNet / MedicalNet ResNet-50 from `torch.hub`) and their input
preparation stay the caller's.  PARITY UNPINNED: upstream's source is not part of the reference; in the full-rank case the value equals
the `sqrtm` form to fp64 rounding.  With x [n, F], y [m, F], Xc / Yc the rows minus their set's mean, G = the Gram matrix of the stacked
rows (centred for FID, raw for MMD and KID) and G_xx, G_yy, G_xy its blocks:

  FID = |mu_x - mu_y|^2 + tr(G_xx) / (n-1) + tr(G_yy) / (m-1) - 2 ||G_xy||_* / sqrt((n-1)(m-1))
  MMD = c1 sum_{i != j} G_yy + c2 sum_{i != j} G_pp - c3 sum G_py,  c1 = 1/(m(m-1)), c2 = 1/(n(n-1)), c3 = 2/(mn)   (y: m rows, y_pred: n)
  KID = sum_{i != j} k_xx / (n(n-1)) + sum_{i != j} k_yy / (m(m-1)) - 2 sum k_xy / (nm),  k = (gamma G + coef0)^degree  (whole sets)

FID's usual form is tr(S_x + S_y - 2 sqrtm(S_x S_y)) with the F x F covariances.  The non-zero eigenvalues of S_x S_y are the squared
singular values of Xc Yc^T / sqrt((n-1)(m-1)), so tr sqrtm(S_x S_y) = ||Xc Yc^T||_* / sqrt((n-1)(m-1)), the nuclear norm of an n x m
block of G: O(nmF) work plus a small SVD instead of a host Schur decomposition of an F x F matrix that is singular whenever n, m <= F
(always, at 2048 features and a few hundred samples).  The identity against numpy cov + `scipy.linalg.sqrtm` in fp64 on the CPU:

  n, m, F         relative difference   rank
  64, 48, 16      1.0e-14               full
  200, 150, 32    4.8e-14               full
  24, 17, 64      2.4e-8                singular  (the residue is sqrtm's)
  40, 40, 128     3.4e-8                singular

Kernels (csrc/distmetrics.hip), fp64 throughout: per-group column means, the Gram matrix on fp64 MFMA tiles over K chunks added in a
fixed order, one-sided Jacobi singular values (round-robin pairs; the host reads a rotation counter once per sweep and stops at the
first sweep without one, at most 60), and a finalize pass per score.  No floating-point atomics: two runs are bit-equal.
"""
from __future__ import annotations

import ctypes as C
import itertools
import math
from collections.abc import Sequence

import torch

from ._lib import call, call_raw, constants, ptr

F32 = torch.float32
MAX_TAPS = 11  # per axis (csrc/metrics.hip: MAXK)
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
_MAX_SCALES = 8


def _per_axis(v, spatial_dims, name):
    if isinstance(v, Sequence) and not isinstance(v, str):
        v = tuple(v)
        if len(v) != spatial_dims:
            raise ValueError(f"{name} has {len(v)} entries, expected one per spatial axis ({spatial_dims})")
        return v
    return (v,) * spatial_dims


def gaussian_taps(k: int, sigma: float) -> list[float]:
    """fp64 taps of one axis: exp(-(t / sigma)^2 / 2) at t = (1 - k) / 2 + i, normalised to sum 1."""
    g = [math.exp(-(((1 - k) / 2 + i) / sigma) ** 2 / 2) for i in range(k)]
    s = sum(g)
    return [v / s for v in g]


def uniform_taps(k: int) -> list[float]:
    return [1.0 / k] * k


def _reduction_ok(r):
    if r not in ("mean", "none"):
        raise NotImplementedError(f"reduction {r!r}: only 'mean' and 'none' are implemented")
    return r


class _SSIMBase:
    levels = 1

    def __init__(self, spatial_dims: int, data_range: float = 1.0, kernel_type: str = "gaussian", kernel_size=11, kernel_sigma=1.5,
                 k1: float = 0.01, k2: float = 0.03, reduction: str = "mean", get_not_nans: bool = False):
        if spatial_dims not in (2, 3):
            raise ValueError(f"spatial_dims must be 2 or 3, got {spatial_dims}")
        if kernel_type not in ("gaussian", "uniform"):
            raise ValueError(f"kernel_type must be 'gaussian' or 'uniform', got {kernel_type!r}")
        self.spatial_dims = spatial_dims
        self.data_range = data_range
        self.kernel_type = kernel_type
        self.kernel_size = _per_axis(kernel_size, spatial_dims, "kernel_size")
        self.kernel_sigma = _per_axis(kernel_sigma, spatial_dims, "kernel_sigma")
        if any(int(k) != k or k < 1 for k in self.kernel_size):
            raise ValueError(f"kernel_size must be positive integers, got {kernel_size}")
        self.kernel_size = tuple(int(k) for k in self.kernel_size)
        self.k1, self.k2 = k1, k2
        self.reduction = _reduction_ok(reduction)
        self.get_not_nans = get_not_nans
        self._buffer: list[torch.Tensor] = []
        self._tap_cache: dict = {}

    # ---------------------------------------------------------------------------------------------------- host-side parameters
    def taps(self) -> list[list[float]]:
        """fp64 taps per spatial axis (axis 0 = D for 3-D, H for 2-D)."""
        if self.kernel_type == "gaussian":
            return [gaussian_taps(k, s) for k, s in zip(self.kernel_size, self.kernel_sigma)]
        return [uniform_taps(k) for k in self.kernel_size]

    def _tap_table(self, device):
        t = self._tap_cache.get(device)
        if t is None:
            axes = self.taps()
            if self.spatial_dims == 2:
                axes = [[1.0]] + axes
            t = torch.tensor([v for a in axes for v in a], dtype=F32).to(device)
            self._tap_cache[device] = t
        return t

    def _constants(self):
        return (self.k1 * self.data_range) ** 2, (self.k2 * self.data_range) ** 2

    def _key(self):
        """Metrics with equal keys share their per-scale sums."""
        return (self.spatial_dims, self.kernel_type, self.kernel_size, tuple(tuple(t) for t in self.taps()), self._constants())

    def _check_shape(self, shape):
        if len(shape) != self.spatial_dims + 2:
            raise ValueError(f"expected {self.spatial_dims + 2}-D input (N, C, spatial...) for spatial_dims={self.spatial_dims}, "
                             f"got shape {tuple(shape)}")
        if any(k > MAX_TAPS for k in self.kernel_size):
            raise NotImplementedError(f"kernel_size {self.kernel_size}: at most {MAX_TAPS} taps per axis on the HIP path")
        sp = shape[2:]
        for e, k in zip(sp, self.kernel_size):
            if e < k:
                raise ValueError(f"spatial extent {tuple(sp)} is smaller than the kernel {self.kernel_size}")

    # ---------------------------------------------------------------------------------------------------- monai buffer semantics
    def __call__(self, y_pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        if y_pred.shape != y.shape:
            raise ValueError(f"y_pred and y must have the same shape, got {tuple(y_pred.shape)} and {tuple(y.shape)}")
        out = _score([y_pred, y], [self], None)[0]
        self._buffer.append(out)
        return out

    def get_buffer(self):
        return torch.cat(self._buffer, 0) if self._buffer else None

    def reset(self):
        self._buffer = []

    def aggregate(self, reduction: str | None = None):
        data = self.get_buffer()
        if not isinstance(data, torch.Tensor):
            raise ValueError("the data to aggregate must be PyTorch Tensor.")
        r = _reduction_ok(reduction or self.reduction)
        nans = torch.isnan(data)
        not_nans = (~nans).float()
        if r == "none":
            return (data, not_nans) if self.get_not_nans else data
        f = torch.where(nans, torch.zeros_like(data), data)
        nn_c = not_nans.sum(dim=1)
        zero = torch.zeros(1, device=f.device, dtype=torch.float)
        f = torch.where(nn_c > 0, f.sum(dim=1).float() / nn_c, zero)
        nn_b = (nn_c > 0).sum(dim=0).float()
        f = torch.where(nn_b > 0, f.sum(dim=0).float() / nn_b, zero)
        return (f, nn_b) if self.get_not_nans else f


class SSIMMetric(_SSIMBase):
    """`generative.metrics.SSIMMetric`: __call__(y_pred, y) -> [B, 1] fp32, the mean SSIM of each batch element (PARITY UNPINNED)."""


class MultiScaleSSIMMetric(_SSIMBase):
    """`generative.metrics.MultiScaleSSIMMetric`: __call__(y_pred, y) -> [B, 1] fp32 (PARITY UNPINNED)."""

    def __init__(self, spatial_dims: int, data_range: float = 1.0, kernel_type: str = "gaussian", kernel_size=11, kernel_sigma=1.5,
                 k1: float = 0.01, k2: float = 0.03, reduction: str = "mean", get_not_nans: bool = False, weights=MS_SSIM_WEIGHTS):
        super().__init__(spatial_dims, data_range, kernel_type, kernel_size, kernel_sigma, k1, k2, reduction, get_not_nans)
        self.weights = tuple(float(w) for w in weights)
        if not 1 <= len(self.weights) <= _MAX_SCALES:
            raise ValueError(f"weights: 1 to {_MAX_SCALES} scales, got {len(self.weights)}")

    @property
    def levels(self):
        return len(self.weights)

    def _check_shape(self, shape):
        super()._check_shape(shape)
        div = max(1, self.levels - 1) ** 2
        sp = shape[2:]
        for e, k in zip(sp, self.kernel_size):
            if e // div <= k - 1:
                raise ValueError(f"for a kernel size of {self.kernel_size} and {self.levels} scales the spatial extent {tuple(sp)} must be "
                                 f"larger than {div * (k - 1)} on every axis (floor(extent / {div}) > kernel size - 1)")
        for s in range(self.levels):  # every scale must still hold the kernel (the rule above does not ensure it above 5 scales)
            if any((e >> s) < k for e, k in zip(sp, self.kernel_size)):
                raise ValueError(f"spatial extent {tuple(sp)} at scale {s} of {self.levels} is smaller than the kernel {self.kernel_size}")


def default_pairs(n: int) -> list[tuple[int, int]]:
    return list(itertools.combinations(range(n), 2))


def pairwise(images: torch.Tensor, *metrics: _SSIMBase, pairs=None) -> tuple[torch.Tensor, ...]:
    """Score every pair (a, b) of `images` (default: itertools.combinations(range(N), 2)) with each metric: one [P, 1] fp32 tensor per
    metric, equal bit for bit to torch.cat([m(images[[a]], images[[b]]) for a, b in pairs]).  The metrics' buffers are not touched."""
    if not metrics:
        raise ValueError("pairwise needs at least one metric")
    pairs = default_pairs(images.shape[0]) if pairs is None else [tuple(int(v) for v in p) for p in pairs]
    n = images.shape[0]
    for a, b in pairs:
        if not (0 <= a < n and 0 <= b < n):
            raise ValueError(f"pair {(a, b)} indexes outside the {n} images")
    return tuple(_score([images], list(metrics), pairs))


# ---------------------------------------------------------------------------------------------------------------- the HIP path
def _prepare(x: torch.Tensor) -> torch.Tensor:
    if not x.is_cuda:
        raise RuntimeError("medical_image_generation_amd metrics run on MI355X only: move the inputs to 'cuda' (no CPU fallback)")
    if not x.is_floating_point():
        raise ValueError(f"SSIM inputs must be floating point, got {x.dtype}")
    if x.dtype != F32:
        x = x.to(F32)
    return x.contiguous()


def _prepare_rows(x: torch.Tensor) -> torch.Tensor:
    if not x.is_cuda:
        raise RuntimeError("medical_image_generation_amd metrics run on MI355X only: move the inputs to 'cuda' (no CPU fallback)")
    return (x if x.dtype == F32 else x.to(F32)).contiguous()


def _dims(shape):
    c, *sp = shape[1:]
    return (c, 1, *sp) if len(sp) == 2 else (c, *sp)


def _pyramid(x: torch.Tensor, levels: int, pool_d: bool) -> list[torch.Tensor]:
    out = [x]
    for _ in range(1, levels):
        cur = out[-1]
        n, (c, d, h, w) = cur.shape[0], _dims(cur.shape)
        shape = (n, c, d // 2, h // 2, w // 2) if pool_d else (n, c, h // 2, w // 2)
        nxt = torch.empty(shape, dtype=F32, device=cur.device)
        call("mi_ssim_pool2", ptr(cur), ptr(nxt), n * c, d, h, w, int(pool_d))
        out.append(nxt)
    return out


def _score(bases: list[torch.Tensor], metrics: list[_SSIMBase], pairs) -> list[torch.Tensor]:
    """bases = [images] with explicit pairs (a, b), or [x, y] scored element by element (pairs None)."""
    for m in metrics:
        if m.spatial_dims != metrics[0].spatial_dims:
            raise ValueError("pairwise: all metrics must have the same spatial_dims")
        m._check_shape(bases[0].shape)
    bases = [_prepare(b) for b in bases]
    dev = bases[0].device
    if pairs is None:
        pairs = [(i, i) for i in range(bases[0].shape[0])]
    P = len(pairs)
    outs = [torch.empty((P, 1), dtype=F32, device=dev) for _ in metrics]
    if P == 0:
        return outs
    pair_t = torch.tensor(pairs, dtype=torch.int32).reshape(P, 2).to(dev)
    levels = max(m.levels for m in metrics)
    pool_d = metrics[0].spatial_dims == 3
    pyr = [_pyramid(b, levels, pool_d) for b in bases]
    xs, ys = pyr[0], pyr[-1]
    groups: dict = {}
    for i, m in enumerate(metrics):
        groups.setdefault(m._key(), []).append(i)
    for idx in groups.values():
        lead = metrics[idx[0]]
        nlev = max(metrics[i].levels for i in idx)
        kd, kh, kw = (1, *lead.kernel_size) if lead.spatial_dims == 2 else lead.kernel_size
        c1, c2 = lead._constants()
        taps = lead._tap_table(dev)
        tiles, counts = [], []
        for s in range(nlev):
            c, d, h, w = _dims(xs[s].shape)
            t = call_raw("mi_ssim_tiles", d, h, w, kd, kh, kw)
            if t <= 0:
                raise ValueError(f"scale {s}: extent {(d, h, w)} does not hold the kernel {(kd, kh, kw)}")
            tiles.append(c * t)
            counts.append(float(c * (d - kd + 1) * (h - kh + 1) * (w - kw + 1)))
        stride = sum(tiles)
        part = torch.empty((P, stride, 2), dtype=torch.float64, device=dev)
        off = 0
        for s in range(nlev):
            c, d, h, w = _dims(xs[s].shape)
            call("mi_ssim_pairs", ptr(xs[s]), ptr(ys[s]), ptr(pair_t), P, c, d, h, w, ptr(taps), kd, kh, kw, c1, c2, ptr(part), stride, off)
            off += tiles[s]
        for i in idx:
            m = metrics[i]
            S = m.levels
            ht = (C.c_int * S)(*tiles[:S])
            hc = (C.c_double * S)(*counts[:S])
            if isinstance(m, MultiScaleSSIMMetric):
                hw = (C.c_double * S)(*m.weights)
                call("mi_ssim_finalize", ptr(part), P, stride, S, ht, hc, hw, ptr(outs[i]), None)
            else:
                call("mi_ssim_finalize", ptr(part), P, stride, S, ht, hc, None, None, ptr(outs[i]))
    return outs


# ------------------------------------------------------------------------------------------------------- FID / MMD / KID
F64 = torch.float64
MAX_JACOBI_SWEEPS = 60  # csrc/distmetrics.hip: MAX_SWEEPS; a bound, not a tuning value (8 to 14 sweeps observed)
_DM_FID, _DM_MMD, _DM_KID = (constants()["MI_DM_" + k] for k in ("FID", "MMD", "KID"))


def _check_features(y_pred: torch.Tensor, y: torch.Tensor):
    if y_pred.ndimension() > 2 or y.ndimension() > 2:
        raise ValueError("Inputs should have (number images, number of features) shape.")
    if y_pred.ndimension() != 2 or y.ndimension() != 2:
        raise ValueError(f"expected two [N, F] feature matrices, got shapes {tuple(y_pred.shape)} and {tuple(y.shape)}")
    if y_pred.shape[1] != y.shape[1] or y.shape[1] < 1:
        raise ValueError(f"the feature widths differ or are empty: {y_pred.shape[1]} and {y.shape[1]}")
    if y_pred.shape[0] < 2 or y.shape[0] < 2:
        raise ValueError(f"each set needs at least 2 rows, got {y_pred.shape[0]} and {y.shape[0]}")
    if not (y_pred.is_floating_point() and y.is_floating_point()):
        raise ValueError(f"feature matrices must be floating point, got {y_pred.dtype} and {y.dtype}")


class _Rows:
    """Two groups of fp32 rows on the device (group 0: n rows, group 1: m rows, K columns each) and what the kernels derive from them."""

    def __init__(self, g0: torch.Tensor, g1: torch.Tensor):
        self.z0, self.z1 = _prepare_rows(g0), _prepare_rows(g1)
        self.n, self.m, self.K = self.z0.shape[0], self.z1.shape[0], self.z0.shape[1]
        self.dev = self.z0.device
        self.sweeps = None

    def colmean(self) -> torch.Tensor:
        mean = torch.empty((2, self.K), dtype=F64, device=self.dev)
        call("mi_dm_colmean", ptr(self.z0), ptr(self.z1), self.n, self.m, self.K, ptr(mean))
        return mean

    def gram(self, mean) -> torch.Tensor:
        R = self.n + self.m
        G = torch.empty((R, R), dtype=F64, device=self.dev)
        ws = torch.empty(call_raw("mi_dm_gram_workspace_bytes", R, self.K) // 8, dtype=F64, device=self.dev)
        call("mi_dm_gram", ptr(self.z0), ptr(self.z1), self.n, self.m, self.K, ptr(mean), ptr(G), ptr(ws))
        return G

    def nuclear_norm(self, G) -> torch.Tensor:
        """Sum of the singular values of G[0:n, n:n+m] (1-element fp64 tensor); the sweeps run are left in self.sweeps."""
        r, c = max(self.n, self.m), min(self.n, self.m)
        cp = c + (c & 1)
        A = torch.empty(r * cp, dtype=F64, device=self.dev)
        counters = torch.empty(MAX_JACOBI_SWEEPS, dtype=torch.int32, device=self.dev)
        call("mi_dm_jacobi_init", ptr(G), self.n, self.m, ptr(A), ptr(counters))
        for sweep in range(MAX_JACOBI_SWEEPS):
            call("mi_dm_jacobi_sweep", ptr(A), r, cp, counters.data_ptr() + 4 * sweep)
            if int(counters[sweep].item()) == 0:  # the one synchronisation of the sweep
                break
        else:
            raise RuntimeError(f"one-sided Jacobi did not converge in {MAX_JACOBI_SWEEPS} sweeps ({r} x {c} block)")
        self.sweeps = sweep + 1
        out = torch.empty(c + 1, dtype=F64, device=self.dev)  # the singular values, then their sum
        call("mi_dm_jacobi_norms", ptr(A), r, c, ptr(out), out.data_ptr() + 8 * c)
        return out[c:]

    def score(self, mode, G, mean=None, nuc=None, degree=1, gamma=1.0, coef0=0.0) -> torch.Tensor:
        out = torch.empty(4, dtype=F64, device=self.dev)  # score and its three terms
        call("mi_dm_finalize", mode, ptr(G), self.n, self.m, ptr(mean), self.K, ptr(nuc), int(degree), float(gamma), float(coef0), ptr(out))
        return out

    def fid(self, mean, G) -> torch.Tensor:
        return self.score(_DM_FID, G, mean=mean, nuc=self.nuclear_norm(G))


class FIDMetric:
    """`generative.metrics.FIDMetric`: __call__(y_pred, y) on two [N, F] feature matrices -> 0-dim fp64 device tensor (PARITY UNPINNED).

    Computed from the Gram matrix of the centred features and the nuclear norm of its cross block (module docstring), not from
    `sqrtm` of the covariance product: that form has no non-finite case, so upstream's `eps * I` offset path does not exist here.
    `last_terms` holds (score, |mu_x - mu_y|^2, tr S_x + tr S_y, 2 tr sqrtm(S_x S_y)) of the last call, `last_sweeps` its Jacobi sweeps."""

    def __init__(self):
        self.last_terms = None
        self.last_sweeps = None

    def __call__(self, y_pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        _check_features(y_pred, y)
        rows = _Rows(y_pred, y)
        mean = rows.colmean()
        self.last_terms = rows.fid(mean, rows.gram(mean))
        self.last_sweeps = rows.sweeps
        return self.last_terms[0]


class MMDMetric:
    """`generative.metrics.MMDMetric`: __call__(y, y_pred) -> 0-dim fp64 device tensor, upstream's linear-kernel estimator on the
    batches flattened to [B, -1] (PARITY UNPINNED).  Deviation: upstream returns the input dtype; the value is a difference of nearly
    equal sums, which an fp32 result would discard, so this returns fp64.  `last_terms`: (score, c1 a, c2 b, c3 c) of the last call."""

    def __init__(self, y_transform=None, y_pred_transform=None):
        self.y_transform = y_transform
        self.y_pred_transform = y_pred_transform
        self.last_terms = None

    def __call__(self, y: torch.Tensor, y_pred: torch.Tensor) -> torch.Tensor:
        if self.y_transform is not None:
            y = self.y_transform(y)
        if self.y_pred_transform is not None:
            y_pred = self.y_pred_transform(y_pred)
        if y_pred.shape != y.shape:
            raise ValueError(f"y_pred and y shapes dont match after being processed by their transforms, received y_pred: {tuple(y_pred.shape)} "
                             f"and y: {tuple(y.shape)}")
        if y.ndimension() < 1 or y.shape[0] < 2:
            raise ValueError(f"MMD needs a batch of at least 2, got shape {tuple(y.shape)}")
        if not (y.is_floating_point() and y_pred.is_floating_point()):
            raise ValueError(f"MMD inputs must be floating point, got {y.dtype} and {y_pred.dtype}")
        if y.numel() == 0:
            raise ValueError(f"MMD inputs are empty: shape {tuple(y.shape)}")
        rows = _Rows(y.reshape(y.shape[0], -1), y_pred.reshape(y_pred.shape[0], -1))
        self.last_terms = rows.score(_DM_MMD, rows.gram(None))
        return self.last_terms[0]


class KIDMetric:
    """Kernel Inception Distance: the unbiased MMD^2 with k(a, b) = (gamma a.b + coef0)^degree over the whole sets (no random subsets:
    deterministic); gamma None = 1 / F.  __call__(y_pred, y) as FIDMetric.  Not part of the reference: PARITY UNPINNED."""

    def __init__(self, degree: int = 3, gamma: float | None = None, coef0: float = 1.0):
        if int(degree) != degree or degree < 1:
            raise ValueError(f"degree must be a positive integer, got {degree}")
        self.degree, self.gamma, self.coef0 = int(degree), gamma, coef0
        self.last_terms = None

    def _score(self, rows: _Rows, G) -> torch.Tensor:
        gamma = 1.0 / rows.K if self.gamma is None else self.gamma
        return rows.score(_DM_KID, G, degree=self.degree, gamma=gamma, coef0=self.coef0)

    def __call__(self, y_pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        _check_features(y_pred, y)
        rows = _Rows(y_pred, y)
        self.last_terms = self._score(rows, rows.gram(None))
        return self.last_terms[0]


def distribution_scores(synth_features: torch.Tensor, real_features: torch.Tensor, kid=True) -> dict:
    """FID and KID of two [N, F] feature matrices in one call, the drop-in for train_ldm.py:308-310: one pass of column means and two
    Gram passes (centred for FID, raw for KID) over the stacked features.  {"fid": 0-dim fp64, "kid": 0-dim fp64, "jacobi_sweeps": int},
    equal bit for bit to FIDMetric()(synth, real) and KIDMetric()(synth, real).  kid: True, False (FID only) or a KIDMetric."""
    _check_features(synth_features, real_features)
    rows = _Rows(synth_features, real_features)
    mean = rows.colmean()
    out = {"fid": rows.fid(mean, rows.gram(mean))[0], "jacobi_sweeps": rows.sweeps}
    if kid:
        metric = kid if isinstance(kid, KIDMetric) else KIDMetric()
        out["kid"] = metric._score(rows, rows.gram(None))[0]
    return out
