"""fp64 restatement of sliding-window inference (monai.inferers.SlidingWindowInferer as this project states it: PARITY UNPINNED),
written from the specification and not from medical_image_generation_amd/sliding.py: window planning, importance maps, padding,
the blend.  Pure torch / numpy on the CPU.

Per axis: image < roi pads to roi, (roi - image) // 2 before and the rest after.  interval = roi when roi == padded image, else
max(int(roi * (1 - overlap)), 1); count = ceil((image - roi) / interval) + 1; start_i = min(i * interval, image - roi).  Windows =
Cartesian product, first axis slowest; flat index n * num_windows + w; runs of sw_batch_size form a call, the last one filled up."""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -24


def axis_plan(image, roi, overlap):
    """(pad_before, pad_after, starts) of one axis."""
    if roi <= 0:
        roi = image
    before = after = 0
    if image < roi:
        before = (roi - image) // 2
        after = roi - image - before
    padded = image + before + after
    interval = roi if roi == padded else max(int(roi * (1 - overlap)), 1)
    count = int(math.ceil((padded - roi) / interval)) + 1
    return before, after, [min(i * interval, padded - roi) for i in range(count)]


def window_starts(image, roi, overlap):
    """-> (pads [(before, after)], starts per axis, windows in enumeration order)."""
    plans = [axis_plan(i, r, overlap) for i, r in zip(image, roi)]
    starts = [p[2] for p in plans]
    windows = [()]
    for st in starts:  # first axis slowest
        windows = [w + (s,) for w in windows for s in st]
    return [(p[0], p[1]) for p in plans], starts, windows


def batches(num_windows, n_images, sw_batch_size):
    """Flat indices per call; None = filler."""
    flat = list(range(num_windows * n_images))
    flat += [None] * (-len(flat) % sw_batch_size)
    return [flat[i:i + sw_batch_size] for i in range(0, len(flat), sw_batch_size)]


def importance(roi, mode, sigma_scale=0.125):
    """float64 tensor."""
    if mode == "constant":
        return torch.ones(tuple(roi), dtype=torch.float64)
    out = torch.ones((), dtype=torch.float64)
    for n in roi:
        i = torch.arange(n, dtype=torch.float64)
        g = torch.exp(-((i - (n - 1) / 2) ** 2) / (2 * (sigma_scale * n) ** 2))
        out = out[..., None] * g
    return out.clamp(min=1e-3)


def nearest(imp, t):
    """imp resampled to extent t with F.interpolate(mode="nearest") itself."""
    return F.interpolate(imp[None, None], size=tuple(t), mode="nearest")[0, 0]


def pad_image(x, pads, mode, cval=0.0):
    """x [N, C, *S] padded per axis by (before, after); torch's own padding modes."""
    flat = []
    for before, after in reversed(pads):
        flat += [before, after]
    if mode == "constant":
        return F.pad(x, flat, mode="constant", value=cval)
    return F.pad(x, flat, mode=mode)


def gather_ref(image, rows, roi, mode, cval):
    """Restatement of the gather: rows (n, z0, y0, x0) count from the image's first voxel, may be negative; n < 0 -> zeros.
    image [N, C, D, H, W] -> [B, C, *roi].  Index arithmetic per axis (no F.pad: origins are arbitrary)."""
    ext = image.shape[2:]

    def src(i, n):
        if 0 <= i < n:
            return i
        if mode == "constant":
            return None
        if mode == "replicate":
            return 0 if i < 0 else n - 1
        return -i if i < 0 else 2 * (n - 1) - i  # reflect, no edge repeat (pad < n)

    out = torch.zeros((len(rows), image.shape[1]) + tuple(roi), dtype=image.dtype)
    for b, (n, z0, y0, x0) in enumerate(rows):
        if n < 0:
            continue
        idx = [[src(o + i, e) for i in range(r)] for o, r, e in zip((z0, y0, x0), roi, ext)]
        tile = torch.full((image.shape[1],) + tuple(roi), float(cval), dtype=image.dtype)
        zi = [(i, s) for i, s in enumerate(idx[0]) if s is not None]
        yi = [(i, s) for i, s in enumerate(idx[1]) if s is not None]
        xi = [(i, s) for i, s in enumerate(idx[2]) if s is not None]
        if zi and yi and xi:
            zs, ys, xs = (torch.tensor([s for _, s in a]) for a in (zi, yi, xi))
            zd, yd, xd = (torch.tensor([i for i, _ in a]) for a in (zi, yi, xi))
            tile[:, zd[:, None, None], yd[None, :, None], xd[None, None, :]] = image[n][:, zs[:, None, None], ys[None, :, None], xs[None, None, :]]
        out[b] = tile
    return out


def blend(preds, imp, origins, n_images, channels, acc_size, crop, final):
    """fp64 blend.  preds: per flat index n * num_windows + w a tensor [Co, *t] (any float dtype); imp [*t]; origins: per window the
    origin in accumulator coordinates.  Returns (out [N, Co, *final], bound [N, Co, *final]): the normalised sum and the fp32 error
    bound (2 K + 4) * 2^-24 * (sum_k w_k |p_k|) / (sum_k w_k) with K the number of windows over the voxel."""
    imp = imp.double()
    acc = torch.zeros((n_images, channels) + tuple(acc_size), dtype=torch.float64)
    mag = torch.zeros_like(acc)
    wsum = torch.zeros(tuple(acc_size), dtype=torch.float64)
    cover = torch.zeros(tuple(acc_size), dtype=torch.float64)
    nw = len(origins)
    for f, p in enumerate(preds):
        n, w = divmod(f, nw)
        sl = tuple(slice(o, o + t) for o, t in zip(origins[w], imp.shape))
        acc[(n, slice(None)) + sl] += imp * p.double()
        mag[(n, slice(None)) + sl] += imp * p.double().abs()
        if n == 0:
            wsum[sl] += imp
            cover[sl] += 1
    sl = tuple(slice(c, c + f) for c, f in zip(crop, final))
    out = acc[(slice(None), slice(None)) + sl] / wsum[sl]
    bound = (2 * cover[sl] + 4) * EPS32 * mag[(slice(None), slice(None)) + sl] / wsum[sl]
    return out, bound


def infer(x, net, roi, overlap, mode="constant", sigma_scale=0.125, padding_mode="constant", cval=0.0):
    """The whole inferer in fp64 bookkeeping around `net` (called per window on fp32 torch slices of the padded image, batch 1).
    Returns per output member (out, bound); a tensor-returning net gives a list of one."""
    n_images = x.shape[0]
    pads, _, windows = window_starts(x.shape[2:], roi, overlap)
    roi = tuple(r if r > 0 else s for r, s in zip(roi, x.shape[2:]))
    xp = pad_image(x, pads, padding_mode, cval)
    imp_in = importance(roi, mode, sigma_scale)
    per_member = None
    for n in range(n_images):
        for w in windows:
            sl = tuple(slice(o, o + r) for o, r in zip(w, roi))
            p = net(xp[(slice(n, n + 1), slice(None)) + sl])
            p = list(p) if isinstance(p, (tuple, list)) else [p]
            if per_member is None:
                per_member = [[] for _ in p]
            for m, t in enumerate(p):
                per_member[m].append(t[0].detach().cpu())
    results = []
    for preds in per_member:
        t = tuple(preds[0].shape[1:])
        ratio = [(tt, r) for tt, r in zip(t, roi)]
        origins = [tuple(o * tt // r for o, (tt, r) in zip(w, ratio)) for w in windows]
        acc_size = tuple(s * tt // r for s, (tt, r) in zip(xp.shape[2:], ratio))
        crop = tuple(pd[0] * tt // r for pd, (tt, r) in zip(pads, ratio))
        final = tuple(s * tt // r for s, (tt, r) in zip(x.shape[2:], ratio))
        imp = nearest(imp_in.float().double(), t) if t != roi else imp_in.float().double()  # the fp32-rounded map, as the product uses
        results.append(blend(preds, imp, origins, n_images, preds[0].shape[0], acc_size, crop, final))
    return results
