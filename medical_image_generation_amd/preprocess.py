"""Case preprocessing on the MI355X: raw array plus spacing in, training case out, on the device.

The reference's planner turns a raw case into a training case on the CPU in fp64 (medimgen/configuration.py:1036-1430:
`resample_image_label`, `crop_image_label`, `normalize_zscore_then_minmax`, `get_sampled_class_locations`, `process_patient`;
preprocess_dataset.py:21-51 is an older form): resample to the dataset's median spacing with `scipy.ndimage.zoom` one axis at a
time (cubic B-spline for images, linear on one-hot channels for labels, order 0 along the low-resolution axis of an anisotropic
case), crop to the non-zero box, transpose (x, y, z[, c]) -> (c, z, y, x), normalise to [0, 1], and store the image, the label and
a properties pickle.  Here the voxel passes are HIP kernels (csrc/preprocess.hip) over fp32 buffers in HBM; what stays on the host
is what is not hot: the per-output-index interpolation taps (fp64, a few hundred numbers per axis) and the sampled class locations.

`scipy.ndimage.zoom(x, [1, n_out / n, 1], order)` with its defaults (mode="constant", prefilter=True, grid_mode=False), restated:
  n_out = int(round(n * zoom));  output o reads u = o * ((n - 1) / (n_out - 1))  (factor 1 when n_out == 1)
  order 0: x[floor(u + 0.5)];  order 1: (1 - t) x[i] + t x[i + 1], i = floor(u), t = u - i
  order 3: the four cubic B-spline weights of t on the prefiltered coefficients c[i - 1 .. i + 2], indices whole-sample mirrored;
  u stays in [0, n - 1], so `cval` is never reached.
The taps are computed here in fp64 and uploaded, so order 0 is a pure gather with scipy's index choice bit for bit.

Not covered: reading NIfTI (pass `np.asarray(img.dataobj)` and the column norms of the affine), writing zarr /
Blosc, the Laplacian-variance quality score, the planner's network sizing.
"""
from __future__ import annotations

import functools
import os
import pickle

import numpy as np
import torch

from ._lib import call, call_raw, ptr

F32 = torch.float32
POLE = np.sqrt(3.0) - 2.0
INIT_HORIZON = 32  # |z|^32 = 5e-19: the causal start's mirror sum is cut here for longer lines, exact for shorter ones
MAX_LABEL_VALUES = 32


# ---------------------------------------------------------------------------------------------------------------- host side, fp64
def resampled_shape(shape, spacing, target_spacing):
    """Spatial shape after resampling `shape` (first three axes) from `spacing` to `target_spacing`: scipy's int(round(n * zoom))
    with zoom = spacing / target (configuration.py:1111)."""
    zoom = np.asarray(spacing, np.float64) / np.asarray(target_spacing, np.float64)
    return tuple(int(round(int(n) * float(z))) for n, z in zip(shape[:3], zoom))


def resample_orders(spacing):
    """Spline order per axis for the image (configuration.py:1101-1123): cubic, and order 0 along the arg-max-spacing axis of an
    anisotropic case (max / min spacing > 3).  The label uses order 1 where this says 3."""
    spacing = np.asarray(spacing, np.float64)
    orders = [3, 3, 3]
    if np.max(spacing) / np.min(spacing) > 3.0:
        orders[int(np.argmax(spacing))] = 0
    return orders


def _mirror(i, n):
    """Whole-sample mirror of index i into [0, n)."""
    if n == 1:
        return 0
    period = 2 * (n - 1)
    i = abs(int(i)) % period
    return period - i if i > n - 1 else i


def axis_taps(n, n_out, order):
    """(idx int32 [n_out, k], w float64 [n_out, k]) with k = 1, 2, 4 for order 0, 1, 3: output o = sum_j w[o, j] * src[idx[o, j]],
    src = the line itself (orders 0, 1) or its cubic B-spline coefficients (order 3).  Indices are resolved (mirrored) into [0, n)."""
    if order not in (0, 1, 3):
        raise ValueError("order must be 0, 1 or 3")
    n, n_out = int(n), int(n_out)
    if n < 1 or n_out < 1:
        raise ValueError("line lengths must be positive")
    k = {0: 1, 1: 2, 3: 4}[order]
    step = (n - 1) / (n_out - 1) if n_out > 1 else 1.0
    idx, w = np.zeros((n_out, k), np.int32), np.zeros((n_out, k), np.float64)
    for o in range(n_out):
        u = step * float(o)
        if order == 0:
            idx[o, 0], w[o, 0] = _mirror(int(np.floor(u + 0.5)), n), 1.0
            continue
        i = int(np.floor(u))
        t = u - i
        if order == 1:
            first, weights = i, (1.0 - t, t)
        else:
            s = 1.0 - t
            w0, w1, w2 = s * s * s / 6.0, (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0, (s * s * (s - 2.0) * 3.0 + 4.0) / 6.0
            first, weights = i - 1, (w0, w1, w2, 1.0 - w0 - w1 - w2)
        for j in range(k):
            idx[o, j], w[o, j] = _mirror(first + j, n), weights[j]
    return idx, w


def prefilter_init_weights(n):
    """Weights of the causal start c[0] = 6 * sum_k w[k] x[k] of the cubic prefilter: the exact whole-sample mirror sum for
    n <= INIT_HORIZON, its first INIT_HORIZON terms otherwise."""
    z = POLE
    if n > INIT_HORIZON:
        return z ** np.arange(INIT_HORIZON, dtype=np.float64)
    k = np.arange(n, dtype=np.float64)
    w = z ** k + z ** (2 * n - 2 - k)
    w[0], w[n - 1] = 1.0, z ** (n - 1)
    return w / (1.0 - z ** (2 * n - 2))


@functools.lru_cache(maxsize=256)
def _tap_tables(n, n_out, order, width):
    """Host tables in the kernels' layout: idx int32 [n_out, width], w fp32 [n_out, width] (unused slots: index of slot 0, weight 0)."""
    idx, w = axis_taps(n, n_out, order)
    k = idx.shape[1]
    full_i, full_w = np.repeat(idx[:, :1], width, axis=1), np.zeros((n_out, width), np.float32)
    full_i[:, :k], full_w[:, :k] = idx, w.astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(full_i)), torch.from_numpy(full_w)


def _zoom_factors(spacing, target_spacing):
    spacing, target = np.asarray(spacing, np.float64), np.asarray(target_spacing, np.float64)
    if spacing.shape != (3,) or target.shape != (3,):
        raise ValueError("spacing and target_spacing must have three entries")
    return spacing, target, spacing / target


def _device_f32(x, what):
    t = torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x)
    if t.is_complex() or t.dtype == torch.bool:
        raise ValueError(f"{what} must have a real dtype")
    if not t.is_cuda:
        t = t.to("cuda")
    return t.to(F32).contiguous()


# -------------------------------------------------------------------------------------------------------------------- device side
def resample_axis(x, axis, n_out, order):
    """One `scipy.ndimage.zoom` axis pass on a contiguous fp32 CUDA tensor: axis `axis` goes from n to n_out samples."""
    n = int(x.shape[axis])
    a = int(np.prod(x.shape[:axis], dtype=np.int64))
    b = int(np.prod(x.shape[axis + 1:], dtype=np.int64))
    src = x
    if order == 3 and n > 1:  # a line of length 1 passes through the prefilter unchanged
        w0 = torch.from_numpy(prefilter_init_weights(n).astype(np.float32)).to(x.device)
        src = torch.empty_like(x)
        call("mi_pp_prefilter3", ptr(x), ptr(src), a, n, b, ptr(w0), int(w0.numel()))
    idx, w = (t.to(x.device) for t in _tap_tables(n, int(n_out), int(order), 4))
    out = torch.empty(tuple(x.shape[:axis]) + (int(n_out),) + tuple(x.shape[axis + 1:]), dtype=F32, device=x.device)
    call("mi_pp_resample_axis", ptr(src), ptr(out), a, n, int(n_out), b, ptr(idx), ptr(w), {0: 1, 1: 2, 3: 4}[int(order)])
    return out


def resample(volume, spacing, target_spacing, orders=None):
    """`resample_image_label`'s image path (configuration.py:1105-1131) on the device: volume (x, y, z) or (x, y, z, c), any real
    dtype (cast to fp32 on upload), resampled along the first three axes one at a time, intermediates staying in HBM.  No resampling
    when np.allclose(spacing, target_spacing); an axis whose zoom factor is exactly 1 is skipped (the reference sends it through
    scipy, where that is the identity up to fp64 rounding).  `orders`: per-axis 0 / 1 / 3, default `resample_orders(spacing)`."""
    x = _device_f32(volume, "volume")
    if x.dim() not in (3, 4):
        raise ValueError("volume must be (x, y, z) or (x, y, z, c)")
    spacing, target, zoom = _zoom_factors(spacing, target_spacing)
    if np.allclose(spacing, target):
        return x
    orders = resample_orders(spacing) if orders is None else [int(o) for o in orders]
    for axis in range(3):
        if zoom[axis] != 1:
            x = resample_axis(x, axis, int(round(int(x.shape[axis]) * float(zoom[axis]))), orders[axis])
    return x


def _label_values(lab, background_competes):
    values = torch.unique(lab).cpu().numpy().astype(np.float64)
    if np.any(values != np.round(values)) or np.any(values < 0) or np.any(values > 255):
        raise ValueError("label values must be integers in [0, 255]")
    if len(values) > MAX_LABEL_VALUES:
        raise ValueError(f"more than {MAX_LABEL_VALUES} distinct label values in one case")
    return values if background_competes else values[values != 0]


def resample_labels(label, spacing, target_spacing, background_competes=True):
    """`resample_image_label`'s label path (configuration.py:1133-1155) in one kernel and without one-hot volumes: label (x, y, z) of
    any real dtype -> uint8 at the resampled shape.  Every label value present in the case is scored by the separable order-1 taps
    on its indicator (order 0 along the low-resolution axis of an anisotropic case) and the best score wins.
      background_competes=True   label 0 is a channel like the others; ties go to the lowest value.
      background_competes=False  the reference as written: argmax over the foreground channels only, so a voxel whose scores are all
                                 zero gets the FIRST FOREGROUND VALUE -- for comparing a run with the reference's files."""
    lab = _device_f32(label, "label")
    if lab.dim() != 3:
        raise ValueError("label must be (x, y, z)")
    spacing, target, zoom = _zoom_factors(spacing, target_spacing)
    values = _label_values(lab, background_competes)
    if np.allclose(spacing, target):
        return lab.to(torch.uint8)
    out_shape = tuple(int(round(int(n) * float(z))) if z != 1 else int(n) for n, z in zip(lab.shape, zoom))
    if len(values) == 0:  # an all-background label with the background left out: nothing to score
        return torch.zeros(out_shape, dtype=torch.uint8, device=lab.device)
    orders = [1 if o == 3 else 0 for o in resample_orders(spacing)]
    tabs = []
    for axis in range(3):
        n = int(lab.shape[axis])
        tabs += [t.to(lab.device) for t in _tap_tables(n, out_shape[axis], orders[axis] if zoom[axis] != 1 else 0, 2)]
    vals = torch.from_numpy(values.astype(np.float32)).to(lab.device)
    out = torch.empty(out_shape, dtype=torch.uint8, device=lab.device)
    call("mi_pp_resample_labels", ptr(lab), ptr(out), ptr(vals), len(values), *[int(s) for s in lab.shape], *out_shape, *[ptr(t) for t in tabs])
    return out


def nonzero_box(x4):
    """`crop_image_label`'s box (configuration.py:1052-1055) of a fp32 CUDA tensor (x, y, z, c): [[lo, hi), ...] per spatial axis over
    all channels.  ValueError when every voxel is zero (the reference fails on the empty min())."""
    box = torch.empty(6, dtype=torch.int32, device=x4.device)
    call("mi_pp_nonzero_box", ptr(x4), *[int(s) for s in x4.shape], ptr(box))
    b = box.cpu().tolist()
    if b[3] < 0:
        raise ValueError("the image is zero everywhere: there is no non-zero box to crop to")
    return [[b[0], b[3] + 1], [b[1], b[4] + 1], [b[2], b[5] + 1]]


def box_stats(x4, box):
    """Per channel inside `box`: float64 [C, 4] = sum, sum of squares, min, max (host array)."""
    c = int(x4.shape[3])
    stats = torch.empty((c, 4), dtype=torch.float64, device=x4.device)
    work = torch.empty(int(call_raw("mi_pp_stats_workspace_bytes", c)) // 8, dtype=torch.float64, device=x4.device)
    lo, size = [b[0] for b in box], [b[1] - b[0] for b in box]
    call("mi_pp_box_stats", ptr(x4), *[int(s) for s in x4.shape], *lo, *size, ptr(stats), ptr(work))
    return stats.cpu().numpy()


def get_sampled_class_locations(label_array, samples_per_slice=50):
    """configuration.py:1352-1380 on a host uint8 (z, y, x) array: {class: [(z, y, x), ...]}, at most `samples_per_slice` voxels per
    class and slice.  Loop order and the `np.random.choice` calls on numpy's global generator are the reference's, so a seeded run
    draws what the reference would."""
    class_locations = {}
    for lbl in np.unique(label_array):
        if lbl == 0:
            continue
        coords = []
        for z in range(label_array.shape[0]):
            found = np.argwhere(label_array[z] == lbl)
            if found.shape[0] == 0:
                continue
            if found.shape[0] > samples_per_slice:
                found = found[np.random.choice(found.shape[0], samples_per_slice, replace=False)]
            coords.extend((z, y, x) for y, x in found)
        class_locations[int(lbl)] = coords
    return class_locations


def preprocess_case(image, spacing, target_spacing, label=None, samples_per_slice=50, background_competes=True):
    """`process_patient` (configuration.py:1383-1430) without the file I/O: resample, crop to the non-zero box, transpose, normalise.

    image: (x, y, z) or (x, y, z, c), numpy or torch, any real dtype.  A 4-D image is resampled per channel -- the reference's scipy
    call raises there (a three-entry zoom on a 4-D array), so multi-channel cases that need resampling have no reference behaviour.
    label: (x, y, z) or None.  Returns a dict:
      'image'       fp32 [C, Z, Y, X] in [0, 1] on the device (`normalize_zscore_then_minmax`, configuration.py:1204-1221; the mean and
                    the deviation cancel: (z - z_min) / (z_max - z_min) = (v - min) / (max - min))
      'label'       uint8 [Z, Y, X] on the device, or None
      'box'         [[lo, hi), ...] along x, y, z of the resampled volume
      'properties'  {'class_locations': {class: [(z, y, x), ...]}, 'min_max': [(min, max) per channel]} -- the reference's .pkl layout
      'mean_std'    [(mean, std) per channel] of the cropped volume (population deviation, as np.std)
    A channel with max == min raises ValueError (the reference would write NaN)."""
    x = _device_f32(image, "image")
    if x.dim() not in (3, 4):
        raise ValueError("image must be (x, y, z) or (x, y, z, c)")
    x = resample(x.unsqueeze(-1) if x.dim() == 3 else x, spacing, target_spacing)
    lab = None
    if label is not None:
        lab = resample_labels(label, spacing, target_spacing, background_competes)
        if tuple(lab.shape) != tuple(x.shape[:3]):
            raise ValueError("image and label must have the same spatial shape")
    box = nonzero_box(x)
    stats = box_stats(x, box)
    lo, size = [b[0] for b in box], [b[1] - b[0] for b in box]
    count = float(np.prod(size, dtype=np.float64))
    vmin, vmax = stats[:, 2], stats[:, 3]
    if np.any(vmax == vmin):
        raise ValueError(f"channel(s) {np.nonzero(vmax == vmin)[0].tolist()} are constant inside the non-zero box: cannot normalise")
    mean = stats[:, 0] / count
    std = np.sqrt(np.maximum(stats[:, 1] / count - mean * mean, 0.0))
    c = int(x.shape[3])
    lo_inv = torch.from_numpy(np.stack([vmin, 1.0 / (vmax - vmin)], axis=1).astype(np.float32)).to(x.device)
    out = torch.empty((c, size[2], size[1], size[0]), dtype=F32, device=x.device)
    call("mi_pp_finish_image", ptr(x), ptr(out), *[int(s) for s in x.shape], *lo, *size, ptr(lo_inv))
    out_label, class_locations = None, {}
    if lab is not None:
        out_label = torch.empty((size[2], size[1], size[0]), dtype=torch.uint8, device=x.device)
        call("mi_pp_finish_label", ptr(lab), ptr(out_label), *[int(s) for s in lab.shape], *lo, *size)
        class_locations = get_sampled_class_locations(out_label.cpu().numpy(), samples_per_slice)
    properties = {"class_locations": class_locations, "min_max": [(np.float64(a), np.float64(b)) for a, b in zip(vmin, vmax)]}
    return {"image": out, "label": out_label, "box": box, "properties": properties, "mean_std": list(zip(mean.tolist(), std.tolist()))}


def save_case(path, name, result, labels_path=None):
    """Write `<name>.npy` (the image) and `<name>.pkl` (the properties) under `path`, where `volume_io.load_image` /
    `ResidentDataset.add_case` find them; with `labels_path`, the label goes to `<labels_path>/<name>.npy`."""
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, name + ".npy"), result["image"].cpu().numpy())
    with open(os.path.join(path, name + ".pkl"), "wb") as f:
        pickle.dump(result["properties"], f)
    if labels_path is not None and result.get("label") is not None:
        os.makedirs(labels_path, exist_ok=True)
        np.save(os.path.join(labels_path, name + ".npy"), result["label"].cpu().numpy())
