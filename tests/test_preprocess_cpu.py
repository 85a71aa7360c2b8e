"""CPU side of the case preprocessing: the fp64 restatement (tests/preprocess_ref.py) and the host-built interpolation taps
(`preprocess.axis_taps`, `prefilter_init_weights`) against `scipy.ndimage.zoom` itself and against a committed fixture of its
results (tests/golden/preprocess_zoom.safetensors, written by tools/gen_preprocess_golden.py), the shape and order rules, the two
label modes on a hand-made case, and the C-ABI surface of csrc/preprocess.hip."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import abi_header
from tests import preprocess_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = (0, 1, 3)
LENGTHS = (1, 2, 3, 5, 33, 40)
FACTORS = (0.37, 0.5, 1.0, 1.5, 2.6)
CASES = [(order, n, f) for order in ORDERS for n in LENGTHS for f in FACTORS if int(round(n * f)) >= 1]
ENTRY_POINTS = ("mi_pp_prefilter3", "mi_pp_resample_axis", "mi_pp_resample_labels", "mi_pp_nonzero_box", "mi_pp_stats_workspace_bytes",
                "mi_pp_box_stats", "mi_pp_finish_image", "mi_pp_finish_label")


def zoom_input(n):
    """[2, n, 2] fp64: the 1-D path runs along the middle axis of a 3-D array"""
    return np.random.default_rng(1000 + n).standard_normal((2, n, 2))


def by_taps(x, n_out, order):
    """the product's host tables applied in fp64 (order 3: on the restatement's exact coefficients)"""
    from medical_image_generation_amd.preprocess import axis_taps
    idx, w = axis_taps(x.shape[1], n_out, order)
    assert idx.dtype == np.int32 and w.dtype == np.float64 and idx.shape == w.shape == (n_out, {0: 1, 1: 2, 3: 4}[order])
    assert idx.min() >= 0 and idx.max() < x.shape[1]
    src = np.moveaxis(R.prefilter(np.moveaxis(x, 1, -1)), -1, 1) if order == 3 else x
    return sum(w[None, :, k, None] * src[:, idx[:, k], :] for k in range(idx.shape[1]))


def check(got, want, order):
    assert got.shape == want.shape
    if order == 0:
        assert np.array_equal(got, want)  # a gather: the index choice is scipy's bit for bit
    else:
        assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("order,n,f", CASES)
def test_restatement_and_taps_match_scipy(order, n, f):
    ndimage = pytest.importorskip("scipy.ndimage")
    x = zoom_input(n)
    want = ndimage.zoom(x, [1, f, 1], order=order)
    assert want.shape[1] == R.out_len(n, f)
    check(R.zoom_axis(x, 1, want.shape[1], order), want, order)
    check(by_taps(x, want.shape[1], order), want, order)


def test_restatement_and_taps_match_the_fixture(golden):
    tensors, meta = golden("preprocess_zoom")
    assert len(tensors) == len(CASES) and "zoom" in meta["call"]
    for order, n, f in CASES:
        want = tensors[f"o{order}_n{n}_f{f}"].numpy()
        assert want.dtype == np.float64 and want.shape == (2, R.out_len(n, f), 2)
        x = zoom_input(n)
        check(R.zoom_axis(x, 1, want.shape[1], order), want, order)
        check(by_taps(x, want.shape[1], order), want, order)


def test_single_output_sample_reads_the_first_input():
    x = zoom_input(5)
    for order in (0, 1):
        assert np.array_equal(R.zoom_axis(x, 1, 1, order), x[:, :1])
    assert np.abs(R.zoom_axis(x, 1, 1, 3) - x[:, :1]).max() <= 1e-12  # a B-spline interpolates its samples


@pytest.mark.parametrize("n", [2, 3, 5, 31, 32, 33, 40, 300])
def test_causal_start_weights(n):
    """exact mirror sum up to the horizon; beyond it the cut terms are below |z|^32 of the line's magnitude"""
    from medical_image_generation_amd.preprocess import INIT_HORIZON, POLE, prefilter_init_weights
    w = prefilter_init_weights(n)
    assert w.dtype == np.float64 and len(w) == min(n, INIT_HORIZON) and POLE == R.Z
    x = np.random.default_rng(n).standard_normal(n)
    zn = R.Z ** (n - 1)
    exact = (x[0] + zn * x[n - 1] + sum(R.Z ** i * (x[i] + zn * x[n - 1 - i]) for i in range(1, n - 1))) / (1 - zn * zn)
    bound = 1e-14 * np.abs(x).max()  # fp64 rounding of a short, geometrically weighted sum
    if n > INIT_HORIZON:
        bound += 2 * abs(R.Z) ** INIT_HORIZON / (1 - abs(R.Z)) * np.abs(x).max()
    assert abs(float(w @ x[:len(w)]) - exact) <= bound
    assert abs(R.Z) ** INIT_HORIZON < 1e-18  # far below fp32 resolution


def test_resampled_shape_and_orders():
    from medical_image_generation_amd.preprocess import resample_orders, resampled_shape
    assert resampled_shape((256, 256, 160), (0.8, 0.8, 2.5), (1, 1, 1)) == (205, 205, 400)
    assert resampled_shape((10, 11, 12, 2), (1.0, 1.0, 4.0), (1.0, 1.0, 1.5)) == (10, 11, 32)
    assert resampled_shape((5, 5, 5), (1.0, 1.0, 1.0), (2.0, 2.0, 2.0)) == (2, 2, 2)  # 2.5 rounds to even: Python's round
    assert resampled_shape((7, 3, 1), (1.0, 1.0, 1.0), (2.0, 2.0, 2.0)) == (4, 2, 0)  # 3.5 -> 4, 1.5 -> 2, 0.5 -> 0
    assert resample_orders((1, 1, 1)) == [3, 3, 3] and R.orders_for((1, 1, 1)) == [3, 3, 3]
    assert resample_orders((1, 1, 3)) == [3, 3, 3]  # the rule is max / min > 3, not >=
    assert resample_orders((1, 1, 3.01)) == [3, 3, 0] == R.orders_for((1, 1, 3.01))
    assert resample_orders((0.5, 4, 1)) == [3, 0, 3] == R.orders_for((0.5, 4, 1))
    assert resample_orders((4, 4, 1)) == [0, 3, 3]  # the first arg-max axis only


def test_label_modes_on_a_hand_made_case():
    """4x4x4, constant over y and z, profile 3 0 0 1 along x, x zoomed by 2: u = o * 3 / 7.  Scores along x
         value 3:  1  .571 .143 0    0    0    0    0
         value 0:  0  .429 .857 1    1    .857 .429 0
         value 1:  0  0    0    0    0    .143 .571 1
    With the background competing the argmax is 3 3 0 0 0 0 1 1; over the foreground channels only (the reference as written) the
    two middle voxels score zero everywhere and get the first foreground value, 1."""
    label = np.zeros((4, 4, 4), np.uint8)
    label[0], label[3] = 3, 1
    got, gap = R.resample_labels(label, (2, 1, 1), (1, 1, 1), background_competes=True)
    assert got.shape == (8, 4, 4) and got.dtype == np.uint8
    assert np.array_equal(got, np.broadcast_to(np.array([3, 3, 0, 0, 0, 0, 1, 1], np.uint8)[:, None, None], got.shape))
    assert np.allclose(gap[:, 0, 0], [1, 1 / 7, 5 / 7, 1, 1, 5 / 7, 1 / 7, 1])
    got, _ = R.resample_labels(label, (2, 1, 1), (1, 1, 1), background_competes=False)
    assert np.array_equal(got, np.broadcast_to(np.array([3, 3, 3, 1, 1, 1, 1, 1], np.uint8)[:, None, None], got.shape))
    # an anisotropic case takes the nearest sample along its low-resolution axis: floor(u + 0.5) of u = 0, 3/7, ... = 0 0 1 1 2 2 3 3
    got, _ = R.resample_labels(label, (4, 1, 1), (2, 1, 1), background_competes=True)
    assert np.array_equal(got[:, 0, 0], [3, 3, 0, 0, 0, 0, 1, 1])
    got, _ = R.resample_labels(label, (4, 1, 1), (2, 1, 1), background_competes=False)
    assert np.array_equal(got[:, 0, 0], [3, 3, 1, 1, 1, 1, 1, 1])
    same, _ = R.resample_labels(label, (1, 1, 1), (1, 1, 1 + 1e-9))
    assert np.array_equal(same, label)  # np.allclose spacings: no resampling


def test_restatement_crop_normalise_and_class_locations():
    vol = np.zeros((6, 5, 4))
    vol[2:5, 1:3, 3] = [[1, 2], [3, 4], [5, 9]]
    assert R.nonzero_box(vol) == [[2, 5], [1, 3], [3, 4]]
    four = np.zeros((6, 5, 4, 2))
    four[0, 4, 0, 1] = -1
    four[3, 2, 2, 0] = 1
    assert R.nonzero_box(four) == [[0, 4], [2, 5], [0, 3]]
    out, min_max = R.normalize(np.array([[1.0, 3.0, 2.0, 5.0]]))
    assert np.allclose(out, [[0, 0.5, 0.25, 1]]) and min_max == [(1.0, 5.0)]
    label = np.zeros((2, 3, 3), np.uint8)
    label[0, 1, :] = 2
    label[1, :, 0] = 7
    np.random.seed(3)
    loc = R.class_locations(label, samples_per_slice=2)
    assert sorted(loc) == [2, 7] and len(loc[2]) == 2 and len(loc[7]) == 2
    assert all(z == 0 and y == 1 for z, y, _ in loc[2]) and all(z == 1 and x == 0 for z, _, x in loc[7])
    from medical_image_generation_amd.preprocess import get_sampled_class_locations
    np.random.seed(3)
    assert get_sampled_class_locations(label, samples_per_slice=2) == loc  # same draws on numpy's global generator


def test_library_exports_the_preprocess_entry_points():
    from medical_image_generation_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    hdr = abi_header.text()
    for name in ENTRY_POINTS:
        assert name in _lib.exported_symbols() and hasattr(lib, name), name
        assert len(abi_header.params(name)) == len(_lib.signature(name)[1]), name  # the binding's argument list is the header's
    assert "resample_image_label 1105-1167" in hdr and "configuration.py:1133-1155" in hdr  # the declarations cite the reference lines they replace
    assert _lib.ABI_VERSION == 20 and lib.mi_abi_version() == 20  # 19 with these entry points; 20: the sampler's step entries became one
    src = open(os.path.join(ROOT, "medical_image_generation_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*:=.*\bpreprocess\.hip\b", src, re.M)


def test_cpu_tensors_and_bad_arguments_are_refused():
    import torch
    from medical_image_generation_amd import preprocess as P
    with pytest.raises(ValueError, match="order"):
        P.axis_taps(5, 7, 2)
    with pytest.raises(ValueError, match="three entries"):
        P._zoom_factors((1, 1), (1, 1, 1))
    if not torch.cuda.is_available():  # no CPU fallback: uploading needs the device
        with pytest.raises((RuntimeError, AssertionError)):
            P.resample(np.zeros((3, 3, 3), np.float32), (1, 1, 2), (1, 1, 1))
