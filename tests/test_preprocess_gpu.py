"""The case-preprocessing kernels (csrc/preprocess.hip) and their Python surface on the GPU, per element against the fp64 restatement
(tests/preprocess_ref.py, itself pinned to scipy.ndimage.zoom by tests/test_preprocess_cpu.py).

Bounds.  Order 0 is a gather: bit-exact.  An order-1 / order-3 axis pass is held to 32 * 2^-24 * max|x| per element: the prefilter's
L1 gain is 3, the two recursions add 1 / (1 - |z|) each, and the result is a four-term dot product; chained passes sum their bounds,
each with max|.| of its own fp64 input.  Every test prints the largest error it saw in those units before it asserts.

LONG = 300 is the line length above every internal size of the kernels: the B == 1 prefilter stages chunks of 64 samples (300 = four
chunks and a tail of 44), and the causal start cuts its mirror sum at 32 terms; 64 and 65 sit on the chunk edge."""
import numpy as np
import pytest
import torch

from tests import preprocess_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PASS_BOUND = 32 * U
LONG = 300
LENGTHS = (1, 2, 3, 5, 33, 64, 65, LONG)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def line_inputs(shape, seed):
    """Gaussian, int16-like CT values in [-1024, 3000], and 0 / 1000 steps -- as fp32 arrays"""
    rng = np.random.default_rng(seed)
    yield "gauss", rng.standard_normal(shape).astype(np.float32)
    yield "ct", rng.integers(-1024, 3001, shape).astype(np.float32)
    yield "steps", (1000.0 * (rng.random(shape) < 0.5)).astype(np.float32)


def out_lengths(n):
    """n_out == 1, down-sampling, the same length through the kernel, up-sampling by 1.5 and 2.6"""
    return sorted({1, max(1, R.out_len(n, 0.37)), n, R.out_len(n, 1.5), R.out_len(n, 2.6)})


def shape_for(position, n):
    # A * B <= 15 lines: the work is in the line length
    return {"middle": (3, n, 5), "last": (15, n), "first": (n, 3, 5)}[position]


@pytest.mark.parametrize("position", ["middle", "last", "first"])  # A, B > 1;  B == 1;  A == 1
@pytest.mark.parametrize("order", [0, 1, 3])
def test_axis_pass(order, position):
    from medical_image_generation_amd.preprocess import resample_axis
    axis = {"middle": 1, "last": 1, "first": 0}[position]
    worst = 0.0
    for n in LENGTHS:
        for kind, x in line_inputs(shape_for(position, n), 7 * n + order):
            xd = dev(x)
            for n_out in out_lengths(n):
                got = resample_axis(xd, axis, n_out, order)
                want = R.zoom_axis(x.astype(np.float64), axis, n_out, order)
                assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
                got = got.cpu().numpy().astype(np.float64)
                if order == 0:
                    assert np.array_equal(got, want), (n, n_out, kind)
                    continue
                err, scale = np.abs(got - want).max(), float(np.abs(x).max())
                worst = max(worst, err / (U * scale) if scale else 0.0)
                assert err <= PASS_BOUND * scale, (n, n_out, kind, err, scale)
            assert torch.equal(xd.cpu(), torch.from_numpy(x))  # the source is never written (the prefilter is out of place)
    print(f"PPERR axis_pass order={order} position={position} max={worst:.2f} units of 2^-24 max|x|")


@pytest.mark.parametrize("order", [1, 3])
def test_axis_pass_many_lines(order):
    """more lines than one workgroup takes: 300 contiguous lines (B == 1: 128 per workgroup) and 3 x 200 columns (256 per workgroup)"""
    from medical_image_generation_amd.preprocess import resample_axis
    worst = 0.0
    for shape, axis in (((300, 70), 1), ((3, 70, 200), 1), ((70, 600), 0)):
        x = np.random.default_rng(shape[0]).standard_normal(shape).astype(np.float32)
        got = resample_axis(dev(x), axis, 93, order).cpu().numpy().astype(np.float64)
        err = np.abs(got - R.zoom_axis(x.astype(np.float64), axis, 93, order)).max() / np.abs(x).max()
        worst = max(worst, err / U)
        assert err <= PASS_BOUND, (shape, err / U)
    print(f"PPERR many_lines order={order} max={worst:.2f} units")


def chained_bound(passes):
    return sum(PASS_BOUND * m for m in passes)


def test_resample_chains_axes_on_the_device():
    from medical_image_generation_amd.preprocess import resample, resampled_shape
    x = np.random.default_rng(5).integers(-1024, 3001, (9, 7, 11)).astype(np.float32)
    for spacing, target, orders in (((1.5, 0.8, 1.34), (1, 1, 1), None), ((2, 2, 2), (1, 1, 1), [1, 1, 1]), ((1, 1, 4), (1, 1, 2), None),
                                    ((1.0, 0.7, 1.0), (1.0, 1.0, 1.0), [3, 1, 0])):
        got = resample(dev(x), spacing, target, orders)
        want, passes = R.resample(x, spacing, target, orders)
        assert tuple(got.shape) == want.shape == resampled_shape(x.shape, spacing, target)
        err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
        print(f"PPERR chain spacing={spacing} err={err:.3e} bound={chained_bound(passes):.3e}")
        assert err <= chained_bound(passes)
    # int16 input is cast on upload; close spacings are not resampled; a 4-D volume goes per channel
    xi = x.astype(np.int16)
    assert torch.equal(resample(xi, (1, 1, 1), (1, 1, 1 + 1e-9)).cpu(), torch.from_numpy(x))
    x4 = np.stack([x, 0.5 * x[::-1]], axis=3)
    got = resample(dev(x4), (1.5, 0.8, 1.34), (1, 1, 1)).cpu().numpy().astype(np.float64)
    for c in range(2):
        want, passes = R.resample(x4[..., c], (1.5, 0.8, 1.34), (1, 1, 1))
        assert np.abs(got[..., c] - want).max() <= chained_bound(passes)


def label_case():
    """12 x 10 x 9, values {0, 1, 2, 5}: two balls and a box"""
    g = np.stack(np.meshgrid(np.arange(12), np.arange(10), np.arange(9), indexing="ij"), axis=0).astype(np.float64)
    lab = np.zeros((12, 10, 9), np.uint8)
    lab[((g[0] - 3.2) ** 2 + (g[1] - 3.1) ** 2 + (g[2] - 3.3) ** 2) < 2.6 ** 2] = 1
    lab[((g[0] - 8.1) ** 2 + (g[1] - 6.2) ** 2 + (g[2] - 5.4) ** 2) < 2.2 ** 2] = 2
    lab[5:8, 1:4, 6:9] = 5
    assert sorted(np.unique(lab)) == [0, 1, 2, 5]
    return lab


@pytest.mark.parametrize("background_competes", [True, False])
@pytest.mark.parametrize("spacing,target", [((1.5, 0.8, 1.34), (1, 1, 1)), ((2, 2, 2), (1, 1, 1)), ((1.5, 0.8, 4.0), (1, 1, 4.0)),
                                            ((1, 1, 4), (1, 1, 1.7))])
def test_labels(spacing, target, background_competes):
    """factors (1.5, 0.8, 1.34), (2, 2, 2), (1.5, 0.8, 1.0) with order 0 on the (untouched) last axis, and (1, 1, 2.35) with order 0
    on the axis that is resampled"""
    from medical_image_generation_amd.preprocess import resample_labels
    lab = label_case()
    got = resample_labels(dev(lab), spacing, target, background_competes)
    want, gap = R.resample_labels(lab, spacing, target, background_competes)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    differ = got.cpu().numpy() != want
    near_tie = gap < 1e-4
    print(f"PPERR labels spacing={spacing} competes={background_competes} differ={int(differ.sum())} near_ties={int(near_tie.sum())} of {want.size}")
    assert not np.any(differ & ~near_tie)
    assert near_tie.sum() <= 0.01 * want.size
    if not background_competes:
        assert np.mean(want == 1) > 0.5  # the reference as written: most of the volume gets the first foreground value


def test_labels_refusals_and_passthrough():
    from medical_image_generation_amd.preprocess import resample_labels
    lab = label_case()
    assert torch.equal(resample_labels(lab, (1, 1, 1), (1, 1, 1)).cpu(), torch.from_numpy(lab))
    many = (np.arange(12 * 10 * 9) % 33).reshape(12, 10, 9)
    with pytest.raises(ValueError, match="32"):
        resample_labels(many, (2, 2, 2), (1, 1, 1))
    with pytest.raises(ValueError, match="integers"):
        resample_labels(lab * 0.5, (2, 2, 2), (1, 1, 1))
    assert resample_labels(np.zeros((4, 4, 4)), (2, 2, 2), (1, 1, 1), background_competes=False).sum().item() == 0


def test_bounding_box():
    from medical_image_generation_amd.preprocess import box_stats, nonzero_box
    x = np.zeros((40, 30, 20, 1), np.float32)  # 24000 voxels: more than one workgroup
    x[3:37, 2:29, 5:19, 0] = np.random.default_rng(0).standard_normal((34, 27, 14)) + 10.0  # every face of the volume is zero
    assert nonzero_box(dev(x)) == [[3, 37], [2, 29], [5, 19]] == R.nonzero_box(x)
    one = np.zeros((40, 30, 20, 1), np.float32)
    one[39, 0, 7] = -1e-30  # a single, tiny, negative voxel in a corner line
    assert nonzero_box(dev(one)) == [[39, 40], [0, 1], [7, 8]]
    two = np.zeros((40, 30, 20, 2), np.float32)
    two[10:20, 10:20, 10:15, 0] = 1.0
    two[0, 29, 19, 1] = 2.0  # only channel 1 reaches the border
    assert nonzero_box(dev(two)) == [[0, 20], [10, 30], [10, 20]] == R.nonzero_box(two)
    with pytest.raises(ValueError, match="zero everywhere"):
        nonzero_box(dev(np.zeros((5, 4, 3, 2), np.float32)))
    # statistics inside a box, per channel, against fp64 numpy
    y = np.random.default_rng(1).standard_normal((40, 30, 20, 2)).astype(np.float32) * 100
    box = [[3, 37], [2, 29], [5, 19]]
    got = box_stats(dev(y), box)
    inner = y[3:37, 2:29, 5:19].astype(np.float64)
    for c in range(2):
        want = [inner[..., c].sum(), (inner[..., c] ** 2).sum(), inner[..., c].min(), inner[..., c].max()]
        assert np.allclose(got[c], want, rtol=1e-12, atol=1e-7), (c, got[c], want)  # fp64 folds of exact fp32 terms
        assert got[c][2] == want[2] and got[c][3] == want[3]


def smooth_ct(shape, seed):
    """CT-like: a smooth field in about [-1000, 1000] plus integer noise"""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.linspace(-1, 1, s) for s in shape], indexing="ij")
    field = 900.0 * np.cos(2.1 * g[0] + 0.3) * np.cos(1.7 * g[1] - 0.2) * np.cos(2.6 * g[2])
    return np.round(field + rng.integers(-100, 101, shape)).astype(np.float32)


def check_case(got, want, image_bounds):
    """box, image per channel within image_bounds[c], min_max within 1e-6 of each value"""
    assert got["box"] == want["box"]
    img = got["image"].cpu().numpy().astype(np.float64)
    assert got["image"].dtype == torch.float32 and img.shape == want["image"].shape and len(image_bounds) == img.shape[0]
    for c, bound in enumerate(image_bounds):
        err = np.abs(img[c] - want["image"][c]).max()
        print(f"PPERR case channel {c} image err={err / U:.2f} units, bound={bound / U:.2f} units")
        assert err <= bound
    assert img.min() >= 0.0 and img.max() <= 1.0
    for (a, b), (c, d) in zip(got["properties"]["min_max"], want["min_max"]):
        print(f"PPERR case min_max got=({a!r}, {b!r}) want=({c!r}, {d!r})")
        assert abs(a - c) <= 1e-6 * abs(c) and abs(b - d) <= 1e-6 * abs(d)


def test_case_without_resampling():
    from medical_image_generation_amd.preprocess import preprocess_case
    img = np.zeros((14, 12, 10), np.float32)
    img[2:11, 3:12, 1:8] = smooth_ct((9, 9, 7), 2) + 2000.0  # non-zero everywhere in the block
    lab = np.zeros((14, 12, 10), np.uint8)
    lab[4:8, 5:9, 2:6] = 3
    lab[8:10, 4:6, 6:8] = 1
    np.random.seed(11)
    got = preprocess_case(img, (1.0, 1.0, 2.0), (1.0, 1.0, 2.0), label=lab, samples_per_slice=3)
    np.random.seed(11)
    want = R.preprocess_case(img, (1.0, 1.0, 2.0), (1.0, 1.0, 2.0), label=lab, samples_per_slice=3)
    assert got["box"] == [[2, 11], [3, 12], [1, 8]]
    check_case(got, want, [4 * U])
    assert got["label"].dtype == torch.uint8 and np.array_equal(got["label"].cpu().numpy(), want["label"])
    assert got["properties"]["class_locations"] == want["class_locations"] and sorted(want["class_locations"]) == [1, 3]
    (mean, std), inner = got["mean_std"][0], img[2:11, 3:12, 1:8].astype(np.float64)
    assert abs(mean - inner.mean()) <= 1e-9 * abs(inner.mean()) and abs(std - inner.std()) <= 1e-6 * inner.std()


def anisotropic_case():
    """spacing (1, 1, 4): zero slabs of 3 voxels at both ends of the low-resolution axis, zero margins of at most 8 voxels elsewhere"""
    img = np.zeros((30, 26, 13), np.float32)
    img[8:25, 3:20, 3:10] = smooth_ct((17, 17, 7), 4)  # both extremes far from 0: min_max is held to 1e-6 of each value
    lab = np.zeros((30, 26, 13), np.uint8)
    g = np.stack(np.meshgrid(np.arange(30), np.arange(26), np.arange(13), indexing="ij"), axis=0).astype(np.float64)
    lab[((g[0] - 14.3) ** 2 + (g[1] - 9.2) ** 2 + 9.0 * (g[2] - 5.1) ** 2) < 4.4 ** 2] = 2
    lab[17:22, 12:17, 6:9] = 4
    return img, lab


def test_case_anisotropic():
    from medical_image_generation_amd.preprocess import preprocess_case, resample_orders
    img, lab = anisotropic_case()
    spacing, target = (1.0, 1.0, 4.0), (0.83, 1.17, 2.3)
    assert resample_orders(spacing) == [3, 3, 0]
    np.random.seed(5)
    got = preprocess_case(img, spacing, target, label=lab, samples_per_slice=4)
    np.random.seed(5)
    want = R.preprocess_case(img, spacing, target, label=lab, samples_per_slice=4)
    (lo, hi), = want["min_max"]
    assert len(want["passes"][0]) == 2  # two cubic passes, the low-resolution axis is a gather
    check_case(got, want, [chained_bound(want["passes"][0]) / (hi - lo)])
    assert want["box"][2][0] > 0 and want["box"][2][1] < R.out_len(13, 4.0 / 2.3)  # the zero slabs are cropped
    differ = got["label"].cpu().numpy() != want["label"]
    print(f"PPERR case labels differ={int(differ.sum())} near_ties={int((want['gap'] < 1e-4).sum())}")
    assert not np.any(want["gap"] < 1e-4)  # this target spacing leaves the restatement without near ties, so the labels must be equal
    assert not np.any(differ)
    assert got["properties"]["class_locations"] == want["class_locations"] and sorted(want["class_locations"]) == [2, 4]


def test_case_two_channels():
    from medical_image_generation_amd.preprocess import preprocess_case
    img = np.zeros((16, 14, 12, 2), np.float32)
    img[2:13, 4:12, 1:9, 0] = smooth_ct((11, 8, 8), 6)
    img[4:15, 2:10, 3:11, 1] = 0.01 * smooth_ct((11, 8, 8), 7)
    spacing, target = (1.0, 1.3, 0.9), (1.1, 1.0, 1.0)
    got = preprocess_case(img, spacing, target)
    want = R.preprocess_case(img, spacing, target)
    assert got["label"] is None and got["properties"]["class_locations"] == {}
    assert got["image"].shape[0] == 2 and [len(p) for p in want["passes"]] == [3, 3]
    check_case(got, want, [chained_bound(p) / (hi - lo) for p, (lo, hi) in zip(want["passes"], want["min_max"])])


def test_dataset_round_trip(tmp_path):
    from medical_image_generation_amd.data import GpuPatchLoader, ResidentDataset
    from medical_image_generation_amd.preprocess import preprocess_case, save_case
    flat = np.zeros((8, 8, 8, 2), np.float32)
    flat[1:7, 1:7, 1:7, 0] = np.random.default_rng(0).standard_normal((6, 6, 6))
    flat[..., 1] = 3.0  # constant over the whole box
    with pytest.raises(ValueError, match="constant"):
        preprocess_case(flat, (1, 1, 1), (1, 1, 1))
    img, lab = anisotropic_case()
    ds = ResidentDataset()
    np.random.seed(2)
    result = ds.add_raw("case0", img, (1.0, 1.0, 4.0), (0.83, 1.17, 2.3), label=lab, samples_per_slice=4)
    ds.add_raw("case1", img[::-1].copy(), (1.0, 1.0, 4.0), (0.83, 1.17, 2.3), label=lab[::-1].copy(), samples_per_slice=4)
    assert len(ds) == 2 and ds.volumes["case0"].shape == result["image"].shape and sorted(ds.class_locations["case0"]) == [2, 4]
    np.random.seed(3)
    loader = GpuPatchLoader(ds, (8, 16, 16), batch_size=2, number_of_steps=2, oversample_foreground_percent=0.5)
    batches = list(loader)
    assert len(batches) == 2 and batches[0]["image"].shape == (2, 1, 8, 16, 16) and sorted(batches[0]["id"]) == ["case0", "case1"]
    assert all(torch.isfinite(b["image"]).all() and b["image"].min() >= 0 and b["image"].max() <= 1 for b in batches)
    assert batches[0]["image"].max() > 0
    save_case(str(tmp_path / "images"), "case0", result, labels_path=str(tmp_path / "labels"))
    back = ResidentDataset()
    back.add_case(str(tmp_path / "images"), "case0")
    assert torch.equal(back.volumes["case0"], ds.volumes["case0"])  # bit for bit
    assert back.class_locations["case0"] == ds.class_locations["case0"]
    assert np.array_equal(np.load(tmp_path / "labels" / "case0.npy"), result["label"].cpu().numpy())
    from medical_image_generation_amd.volume_io import load_image
    image, properties = load_image(str(tmp_path / "images"), "case0")
    assert np.array_equal(np.asarray(image), result["image"].cpu().numpy()) and properties["min_max"] == result["properties"]["min_max"]
