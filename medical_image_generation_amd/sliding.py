"""Sliding-window inference on the MI355X: a patch-trained network run over a whole case.

The reference trains its autoencoder on patches (`ae_transformations.patch_size`, train_autoencoder.py:597, train_ldm.py:518), and
the cases `preprocess.py` produces are whole volumes, usually larger than the patch.  The MONAI ecosystem the reference is built on
answers this with `monai.inferers.SlidingWindowInferer`; `SlidingWindowInferer` / `sliding_window_inference` here are the swap for
it.  MONAI is not part of the reference tree, so the semantics below are restated from MONAI 1.x as recalled and are UNPINNED
(PARITY UNPINNED): the tests pin the kernels and the planner against an fp64 restatement of this text (tests/sliding_ref.py), not
against MONAI.

Per spatial axis, for an image extent `image`, a window extent `roi` (an entry <= 0 means `image`) and `0 <= overlap < 1`:
  padding    image < roi: the image is padded to roi, (roi - image) // 2 voxels before and the rest after (`padding_mode`, `cval`);
  interval   roi when roi equals the (padded) image extent, else max(int(roi * (1 - overlap)), 1);
  windows    count = ceil((image - roi) / interval) + 1, start_i = min(i * interval, image - roi): the last one is shifted back inside.
Windows are the Cartesian product of the per-axis starts, first spatial axis slowest; the flat index over a batch of N images is
n * num_windows + w, consecutive runs of `sw_batch_size` flat indices form one network call, and the last call is filled up with
filler rows (zeros in, nothing accumulated), so every call has one shape: one conv-plan set, one graph.

Importance map (fp64 on the host, rounded once to fp32): "constant" is all ones; "gaussian" is the outer product over the axes of
exp(-(i - (n - 1) / 2)^2 / (2 (sigma_scale n)^2)), not rescaled, floored at 1e-3.

The network's output may have another spatial extent t than roi (latents when encoding, images when decoding).  Per axis t / roi must
map every window start, the padded image extent, the image extent and the padding in front of it to integers (ValueError otherwise);
the output's importance map is the input one resampled as F.interpolate(mode="nearest") does, index floor(j * roi / t).  A network
that returns a tuple or list is blended per member, each with its own extent.

    out[n, c, v] = (sum_k imp[v - o_k] * pred_k[c, v - o_k]) / (sum_k imp[v - o_k])      over the windows k that cover v, in flat order

The voxel passes are HIP kernels (csrc/sliding.hip): `mi_sw_gather` cuts a window batch out of the image and pads on the fly,
`mi_sw_accumulate` blends one batch of predictions (one launch per window in stream order: no float atomics, the sum is in
enumeration order whatever `sw_batch_size` is), `mi_sw_finish` divides and crops.  Window origins AND the extents of the image and of
the accumulators are read from a device table, never from launch arguments.

`use_graph=True` captures gather -> network -> accumulate once per (network, channel count, extra arguments) and replays it for
every window batch after copying that batch's rows into the static table the graph points at (device to device: all batches of a
case are uploaded in one transfer).  The image, the accumulators and the weight sums are static flat buffers whose extents come from
that table, so one graph serves every case whatever its extent or batch size; the buffers have the capacity of the largest case seen,
and only a case with more voxels than every earlier one allocates larger buffers and captures again.  Eager and captured results are
bit-equal: the same launches in the same order.

Not covered (NotImplementedError names the keyword): padding_mode="circular", a `sw_device` / `device` other than the inputs',
`roi_weight_map`, `process_fn`, `buffer_steps`.
"""
from __future__ import annotations

import itertools
import math

import numpy as np
import torch

from . import hipops as ops
from ._lib import call, constants, ptr

F32 = torch.float32
PAD_MODES = {k: constants()["MI_SW_PAD_" + k.upper()] for k in ("constant", "reflect", "replicate")}
GAUSSIAN_FLOOR = 1e-3


# ---------------------------------------------------------------------------------------------------------------- host side, fp64
def _per_axis(value, nd, what, cast=float):
    if isinstance(value, (tuple, list)):
        if len(value) != nd:
            raise ValueError(f"{what} must have one entry per spatial axis ({nd}), got {len(value)}")
        return tuple(cast(v) for v in value)
    return (cast(value),) * nd


def axis_windows(image, roi, overlap):
    """One axis: (roi, pad_before, padded extent, starts) as the module docstring states them."""
    image, roi = int(image), int(roi)
    if image < 1:
        raise ValueError("image extents must be positive")
    if not 0 <= overlap < 1:
        raise ValueError(f"overlap must lie in [0, 1), got {overlap}")
    if roi <= 0:
        roi = image
    padded = max(image, roi)
    pad_before = (roi - image) // 2 if image < roi else 0
    interval = roi if roi == padded else max(int(roi * (1 - overlap)), 1)
    count = -((padded - roi) // -interval) + 1
    return roi, pad_before, padded, [min(i * interval, padded - roi) for i in range(count)]


class WindowPlan:
    """The windows of one case: `roi`, `pad_before`, `padded` and `starts` per axis; `windows` = the origins in padded coordinates in
    enumeration order (first spatial axis slowest)."""

    def __init__(self, image_size, roi_size, overlap):
        nd = len(image_size)
        roi_size = _per_axis(roi_size, nd, "roi_size", int)
        overlap = _per_axis(overlap, nd, "overlap")
        axes = [axis_windows(s, r, o) for s, r, o in zip(image_size, roi_size, overlap)]
        self.image = tuple(int(s) for s in image_size)
        self.roi = tuple(a[0] for a in axes)
        self.pad_before = tuple(a[1] for a in axes)
        self.padded = tuple(a[2] for a in axes)
        self.starts = [a[3] for a in axes]
        self.windows = list(itertools.product(*self.starts))

    @property
    def num_windows(self):
        return len(self.windows)

    def rows(self, n_images, sw_batch_size):
        """int32 [calls, sw_batch_size, 1 + nd]: (n, *origin in padded coordinates) of flat index n * num_windows + w, the last call
        filled up with filler rows (n = -1)."""
        b = int(sw_batch_size)
        if b < 1:
            raise ValueError("sw_batch_size must be at least 1")
        flat = [(n,) + w for n in range(int(n_images)) for w in self.windows]
        flat += [(-1,) + (0,) * len(self.roi)] * (-len(flat) % b)
        return np.asarray(flat, np.int32).reshape(len(flat) // b, b, 1 + len(self.roi))

    def scaled(self, out_size):
        """For a network output of spatial extent `out_size` per window: (accumulator extent, crop origin, final extent); a window
        start s lies at s * t // roi.  ValueError when t / roi maps a start, the padded extent, the image extent or the padding in
        front of it to no integer."""
        if len(out_size) != len(self.roi):
            raise ValueError(f"the network returned {len(out_size)} spatial axes for windows of {len(self.roi)}")

        def scale(v, t, r, what):
            if (v * t) % r:
                raise ValueError(f"output extent {t} per window of {r}: {what} {v} maps to no whole output voxel")
            return v * t // r

        acc, crop, final = [], [], []
        for t, r, pad, padded, image, st in zip(out_size, self.roi, self.pad_before, self.padded, self.image, self.starts):
            t = int(t)
            if t < 1:
                raise ValueError("the network returned an empty output")
            acc.append(scale(padded, t, r, "the padded image extent"))
            crop.append(scale(pad, t, r, "the padding in front of the image"))
            final.append(scale(image, t, r, "the image extent"))
            for s in st:
                scale(s, t, r, "the window start")
        return tuple(acc), tuple(crop), tuple(final)


def importance_map(roi, mode="constant", sigma_scale=0.125):
    """float64 numpy array of shape `roi`."""
    roi = tuple(int(r) for r in roi)
    if mode == "constant":
        return np.ones(roi, np.float64)
    if mode != "gaussian":
        raise ValueError(f"mode must be 'constant' or 'gaussian', got {mode!r}")
    sig = _per_axis(sigma_scale, len(roi), "sigma_scale")
    out = np.ones((), np.float64)
    for n, s in zip(roi, sig):
        i = np.arange(n, dtype=np.float64)
        out = np.multiply.outer(out, np.exp(-((i - (n - 1) / 2.0) ** 2) / (2.0 * (s * n) ** 2)))
    return np.maximum(out, GAUSSIAN_FLOOR)


def resample_nearest(imp, out_size):
    """`imp` at another extent, as F.interpolate(mode="nearest"): index floor(j * n / t) per axis."""
    for axis, t in enumerate(out_size):
        n = imp.shape[axis]
        imp = np.take(imp, (np.arange(int(t), dtype=np.int64) * n) // int(t), axis=axis)
    return imp


def _dims3(sp):
    return (1,) * (3 - len(sp)) + tuple(int(s) for s in sp)


def _rows3(rows, nd):
    """[..., 1 + nd] -> [..., 4]: a D = 1 axis in front of 2-D origins."""
    if nd == 3:
        return rows
    out = np.zeros(rows.shape[:-1] + (4,), np.int32)
    out[..., 0], out[..., 2:] = rows[..., 0], rows[..., 1:]
    return out


def _net_key(network):
    """What identifies a network across calls: a bound method is a new object at every attribute access."""
    owner = getattr(network, "__self__", None)
    return (id(owner), getattr(network, "__func__", None)) if owner is not None else (id(network), None)


# -------------------------------------------------------------------------------------------------------------------- device side
class _Member:
    """One output of the network: its window extent, accumulator geometry, importance map and buffers."""

    def __init__(self, plan, shape, imp):
        """shape: the member's (channels, *window extent); imp(t): the importance map at that extent, fp32 on the device."""
        self.channels, self.t, self.roi = int(shape[0]), tuple(int(s) for s in shape[1:]), plan.roi
        self.acc_size, self.crop, self.final = plan.scaled(self.t)
        self.imp = imp(self.t)

    def out_rows(self, rows):
        """Input rows [calls, B, 1 + nd] (padded coordinates) -> this member's rows in accumulator coordinates (`scaled` checked
        that every start maps to a whole voxel; filler rows stay at 0)."""
        out = rows.copy()
        out[..., 1:] = rows[..., 1:] * np.asarray(self.t, np.int32) // np.asarray(self.roi, np.int32)
        return out

    def elems(self, n):
        return n * self.channels * math.prod(self.acc_size)


class _Captured:
    """One captured gather -> network -> accumulate and the static buffers it points at."""

    def __init__(self):
        self.graph = None
        self.captures = 0
        self.image = self.table = self.tiles = None
        self.acc, self.wsum, self.imp = [], [], []
        self.shapes = None   # per member (channels, *window extent): what the graph's accumulate launches were captured with
        self.is_seq = False  # the network returns a tuple / list
        self.pinned = None
        self.arena = None


class SlidingWindowInferer:
    """`monai.inferers.SlidingWindowInferer` on the HIP path (module docstring: semantics, PARITY UNPINNED).

    roi_size: window extent per spatial axis (an int applies to every axis; <= 0: the image extent).  overlap, sigma_scale: a number
    or one per axis.  mode: "constant" | "gaussian".  padding_mode: "constant" (`cval`) | "reflect" | "replicate", used where the
    image is smaller than the window.  use_graph: captured mode.  progress is accepted and ignored.
    The call runs under torch.no_grad()."""

    def __init__(self, roi_size, sw_batch_size=1, overlap=0.25, mode="constant", sigma_scale=0.125, padding_mode="constant", cval=0.0,
                 use_graph=False, sw_device=None, device=None, progress=False, roi_weight_map=None, process_fn=None, buffer_steps=None):
        for name, value in (("roi_weight_map", roi_weight_map), ("process_fn", process_fn), ("buffer_steps", buffer_steps)):
            if value is not None:
                raise NotImplementedError(f"{name} is not supported by the HIP sliding-window inferer")
        if padding_mode == "circular":
            raise NotImplementedError("padding_mode='circular' is not supported by the HIP sliding-window inferer")
        if padding_mode not in PAD_MODES:
            raise ValueError(f"padding_mode must be one of {sorted(PAD_MODES)}, got {padding_mode!r}")
        if mode not in ("constant", "gaussian"):
            raise ValueError(f"mode must be 'constant' or 'gaussian', got {mode!r}")
        if int(sw_batch_size) < 1:
            raise ValueError("sw_batch_size must be at least 1")
        for o in (overlap if isinstance(overlap, (tuple, list)) else (overlap,)):
            if not 0 <= float(o) < 1:
                raise ValueError(f"overlap must lie in [0, 1), got {o}")
        self.roi_size, self.sw_batch_size, self.overlap = roi_size, int(sw_batch_size), overlap
        self.mode, self.sigma_scale, self.padding_mode, self.cval = mode, sigma_scale, padding_mode, float(cval)
        self.use_graph = bool(use_graph)
        self.sw_device, self.device = sw_device, device
        self._graphs = {}  # (network, channels, extra arguments) -> _Captured
        self._imps = {}    # (roi, extent, mode, sigma_scale, device) -> the importance map at that extent, fp32 on the device

    # ------------------------------------------------------------------ planning
    def plan(self, image_size):
        return WindowPlan(image_size, self.roi_size, self.overlap)

    def _check_devices(self, inputs):
        for name in ("sw_device", "device"):
            want = getattr(self, name)
            if want is None:
                continue
            want, have = torch.device(want), inputs.device
            if want.type != have.type or (want.index is not None and have.index is not None and want.index != have.index):
                raise NotImplementedError(f"{name}={want} differs from the inputs' device {have}: windows, network and blend share "
                                          "one device here")

    def _importance(self, roi, device):
        """t -> the importance map of windows `roi` resampled to extent t, built once per extent (fp64 on the host, rounded once)."""
        def at(t):
            sigma = tuple(self.sigma_scale) if isinstance(self.sigma_scale, (tuple, list)) else self.sigma_scale
            key = (roi, t, self.mode, sigma, device)
            if key not in self._imps:
                imp = resample_nearest(importance_map(roi, self.mode, self.sigma_scale), t).astype(np.float32)
                self._imps[key] = torch.from_numpy(np.ascontiguousarray(imp)).to(device)
            return self._imps[key]
        return at

    # ------------------------------------------------------------------ kernels
    def _gather(self, image, image_elems, channels, table, host_table, roi3, tiles):
        call("mi_sw_gather", ptr(image), image_elems, channels, ptr(table), None if host_table is None else host_table.data_ptr(),
             self.sw_batch_size, *roi3, PAD_MODES[self.padding_mode], self.cval, ptr(tiles))

    def _accumulate(self, pred, member_imp, table, host_table, acc, wsum, acc_elems):
        call("mi_sw_accumulate", ptr(pred), ptr(member_imp), ptr(table), None if host_table is None else host_table.data_ptr(),
             self.sw_batch_size, int(pred.shape[1]), *_dims3(pred.shape[2:]), ptr(acc), ptr(wsum), acc_elems)

    @staticmethod
    def _as_members(pred):
        members = list(pred) if isinstance(pred, (tuple, list)) else [pred]
        for p in members:
            if not torch.is_tensor(p) or not p.is_cuda:
                raise TypeError("the network must return a CUDA tensor or a tuple / list of them")
        return [p.to(F32).contiguous() for p in members], isinstance(pred, (tuple, list))

    # ------------------------------------------------------------------ the call
    @torch.no_grad()
    def __call__(self, inputs, network, *args, **kwargs):
        self._check_devices(inputs)
        if not inputs.is_cuda:
            raise RuntimeError("medical_image_generation_amd runs on MI355X only: move the inputs to 'cuda' (there is no CPU fallback)")
        if inputs.dim() not in (4, 5):
            raise ValueError("inputs must be [N, C, H, W] or [N, C, D, H, W]")
        x = inputs.to(F32).contiguous()  # cast once
        n, c, sp = int(x.shape[0]), int(x.shape[1]), tuple(int(s) for s in x.shape[2:])
        nd = len(sp)
        plan = self.plan(sp)
        if self.padding_mode == "reflect":
            for s, p in zip(sp, plan.padded):
                if p - s - (p - s) // 2 >= s:  # the larger of the two pads
                    raise ValueError(f"padding_mode='reflect' cannot pad an axis of {s} voxels to {p}")
        rows = plan.rows(n, self.sw_batch_size)
        imp = self._importance(plan.roi, x.device)
        roi3 = _dims3(plan.roi)
        # gather rows count from the image's first voxel: padded coordinates minus the padding in front
        g_rows = rows.copy()
        g_rows[..., 1:] -= np.asarray(plan.pad_before, np.int32)
        g_rows[rows[..., 0] < 0, 1:] = 0
        head_in = np.asarray([n] + list(_dims3(sp)), np.int32)
        run = self._run_graph if self.use_graph else self._run_eager
        outs, is_seq = run(x, network, args, kwargs, plan, rows, _rows3(g_rows, nd), head_in, imp, roi3)
        return tuple(outs) if is_seq else outs[0]

    def _tables(self, head_in, g_rows3, members, rows, n, nd):
        """int32 [calls, 1 + M, 1 + B, 4] on the host: per call the gather table, then one accumulate table per member."""
        calls, b = g_rows3.shape[:2]
        tab = np.zeros((calls, 1 + len(members), 1 + b, 4), np.int32)
        tab[:, 0, 0], tab[:, 0, 1:] = head_in, g_rows3
        for m, mem in enumerate(members):
            tab[:, 1 + m, 0] = np.asarray([n] + list(_dims3(mem.acc_size)), np.int32)
            tab[:, 1 + m, 1:] = _rows3(mem.out_rows(rows), nd)
        return torch.from_numpy(tab)

    def _finish(self, members, accs, wsums, n):
        outs = []
        for mem, acc, wsum in zip(members, accs, wsums):
            out = torch.empty((n, mem.channels) + mem.final, dtype=F32, device=acc.device)
            crop3 = (0,) * (3 - len(mem.crop)) + mem.crop
            call("mi_sw_finish", ptr(acc), ptr(wsum), ptr(out), n, mem.channels, *_dims3(mem.acc_size), *crop3, *_dims3(mem.final))
            outs.append(out)
        return outs

    def _run_eager(self, x, network, args, kwargs, plan, rows, g_rows3, head_in, imp, roi3):
        n, c, nd, dev = int(x.shape[0]), int(x.shape[1]), len(plan.roi), x.device
        b = self.sw_batch_size
        tiles = torch.empty((b, c) + plan.roi, dtype=F32, device=dev)
        first = torch.from_numpy(np.concatenate([head_in[None], g_rows3[0]]))
        self._gather(x, x.numel(), c, first.to(dev), first, roi3, tiles)
        preds, is_seq = self._as_members(network(tiles, *args, **kwargs))
        members = [_Member(plan, p.shape[1:], imp) for p in preds]
        host = self._tables(head_in, g_rows3, members, rows, n, nd)
        tables = host.to(dev)
        accs = [torch.zeros((n, m.channels) + m.acc_size, dtype=F32, device=dev) for m in members]
        wsums = [torch.zeros(m.acc_size, dtype=F32, device=dev) for m in members]
        for k in range(host.shape[0]):
            if k:
                self._gather(x, x.numel(), c, tables[k, 0], host[k, 0], roi3, tiles)
                preds, _ = self._as_members(network(tiles, *args, **kwargs))
            for m, (mem, p) in enumerate(zip(members, preds)):
                if tuple(p.shape[1:]) != (mem.channels,) + mem.t:
                    raise RuntimeError("the network's output shape changed between window batches")
                self._accumulate(p, mem.imp, tables[k, 1 + m], host[k, 1 + m], accs[m], wsums[m], accs[m].numel())
        return self._finish(members, accs, wsums, n), is_seq

    # ------------------------------------------------------------------ captured mode
    def _body(self, cap, network, args, kwargs, c, roi3, accumulate=True):
        """gather -> network -> accumulate on the static buffers of `cap`; host tables are not given: the kernels guard themselves."""
        self._gather(cap.image, cap.image.numel(), c, cap.table[0], None, roi3, cap.tiles)
        preds, is_seq = self._as_members(network(cap.tiles, *args, **kwargs))
        if accumulate:
            for m, p in enumerate(preds):
                self._accumulate(p, cap.imp[m], cap.table[1 + m], None, cap.acc[m], cap.wsum[m], cap.acc[m].numel())
        return preds, is_seq

    def _run_graph(self, x, network, args, kwargs, plan, rows, g_rows3, head_in, imp, roi3):
        n, c, nd, dev = int(x.shape[0]), int(x.shape[1]), len(plan.roi), x.device
        b = self.sw_batch_size
        key = (_net_key(network), c, plan.roi, tuple(id(a) for a in args), tuple((k, id(v)) for k, v in sorted(kwargs.items())))
        cap = self._graphs.get(key)
        if cap is None:
            cap = self._graphs[key] = _Captured()
        owner = getattr(network, "__self__", network)
        if cap.graph is not None and getattr(owner, "_arena", None) is not cap.arena:  # the module moved: the graph points at old buffers
            cap.graph = None
        if cap.image is None or cap.image.numel() < x.numel():
            cap.image, cap.graph = torch.empty(x.numel(), dtype=F32, device=dev), None
        if cap.tiles is None:
            cap.tiles = torch.empty((b, c) + plan.roi, dtype=F32, device=dev)
        cap.image[:x.numel()].copy_(x.reshape(-1))
        # shapes of the outputs: a warm-up call on the first gathered batch, nothing accumulated (it also creates conv plans and
        # workspaces outside the capture)
        first = torch.from_numpy(np.concatenate([head_in[None], g_rows3[0]]))
        if cap.table is None:
            cap.table = torch.zeros((1, 1 + b, 4), dtype=torch.int32, device=dev)
        cap.table[0].copy_(first)
        if cap.graph is None:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):  # the second pass packs the weights of the plans the first one created in one batch
                    preds, is_seq = self._body(cap, network, args, kwargs, c, roi3, accumulate=False)
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            cap.shapes, cap.is_seq = [tuple(p.shape[1:]) for p in preds], is_seq
            del preds
        members = [_Member(plan, shape, imp) for shape in cap.shapes]
        if cap.table.shape[0] != 1 + len(members):
            table = torch.zeros((1 + len(members), 1 + b, 4), dtype=torch.int32, device=dev)
            table[0].copy_(cap.table[0])
            cap.table, cap.graph = table, None
        for m, mem in enumerate(members):
            if len(cap.acc) <= m:
                cap.acc.append(None), cap.wsum.append(None), cap.imp.append(None)
            if cap.acc[m] is None or cap.acc[m].numel() < mem.elems(n):
                cap.acc[m], cap.graph = torch.empty(mem.elems(n), dtype=F32, device=dev), None
            if cap.wsum[m] is None or cap.wsum[m].numel() < math.prod(mem.acc_size):
                cap.wsum[m], cap.graph = torch.empty(math.prod(mem.acc_size), dtype=F32, device=dev), None
            if cap.imp[m] is None:
                cap.imp[m] = torch.empty_like(mem.imp)
            cap.imp[m].copy_(mem.imp)
            cap.acc[m][:mem.elems(n)].zero_()
            cap.wsum[m][:math.prod(mem.acc_size)].zero_()
        tables = self._tables(head_in, g_rows3, members, rows, n, nd).to(dev)
        if cap.graph is None:
            cap.table.copy_(tables[0])
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                self._body(cap, network, args, kwargs, c, roi3)
            cap.graph, cap.captures = graph, cap.captures + 1
            cap.arena = getattr(owner, "_arena", None)
            # keep what the graph points at alive: conv plans, the weight-pack batch, the arena, GroupNorm / attention workspaces
            cap.pinned = (dict(getattr(owner, "_plans", {})), getattr(owner, "_packb", None), cap.arena, dict(ops._ws_cache), args, kwargs)
        for k in range(tables.shape[0]):
            cap.table.copy_(tables[k])  # this batch's rows (and the case's extents) into the table the graph reads
            cap.graph.replay()
        accs = [cap.acc[m][:mem.elems(n)] for m, mem in enumerate(members)]
        return self._finish(members, accs, cap.wsum, n), cap.is_seq


def sliding_window_inference(inputs, roi_size, sw_batch_size, predictor, overlap=0.25, mode="constant", sigma_scale=0.125,
                             padding_mode="constant", cval=0.0, sw_device=None, device=None, progress=False, roi_weight_map=None,
                             process_fn=None, buffer_steps=None, *args, **kwargs):
    """`monai.inferers.sliding_window_inference` (function form, eager): see SlidingWindowInferer."""
    inferer = SlidingWindowInferer(roi_size, sw_batch_size, overlap, mode, sigma_scale, padding_mode, cval, False, sw_device, device,
                                   progress, roi_weight_map, process_fn, buffer_steps)
    return inferer(inputs, predictor, *args, **kwargs)


# ------------------------------------------------------------------------------------------------------------- autoencoder helpers
def tiled_reconstruct(ae, x, inferer):
    """`ae.reconstruct` window by window: decode(z_mu) of every window, blended in image space."""
    return inferer(x, ae.reconstruct)


def tiled_encode(ae, x, inferer):
    """`ae.encode` window by window -> (z_mu, z_sigma), each blended on the latent grid."""
    z_mu, z_sigma = inferer(x, ae.encode)
    return z_mu, z_sigma


def tiled_decode(ae, z, inferer):
    """`ae.decode` window by window; the inferer's roi_size is in latent voxels."""
    return inferer(z, ae.decode)
