"""Host side of sliding-window inference (medical_image_generation_amd/sliding.py): window planning, importance maps, output
extents, refusals -- against hand-checked tables and the fp64 restatement tests/sliding_ref.py.  No GPU."""
import numpy as np
import pytest
import torch

from tests import sliding_ref as R

# image, roi, overlap, starts per axis, windows, (pad before, pad after) per axis
TABLE = [
    ((13, 18, 23), (8, 8, 16), 0.25, [[0, 5], [0, 6, 10], [0, 7]], 12, [(0, 0)] * 3),
    ((5, 18, 23), (8, 8, 16), 0.5, [[0], [0, 4, 8, 10], [0, 7]], 8, [(1, 2), (0, 0), (0, 0)]),
    ((16, 24, 32), (8, 16, 16), 0.5, [[0, 4, 8], [0, 8], [0, 8, 16]], 18, [(0, 0)] * 3),
    ((16, 16, 16), (16, 16, 16), 0.25, [[0], [0], [0]], 1, [(0, 0)] * 3),
]


@pytest.mark.parametrize("image,roi,overlap,starts,count,pads", TABLE)
def test_window_starts_match_the_hand_checked_table(image, roi, overlap, starts, count, pads):
    from medical_image_generation_amd.sliding import WindowPlan
    plan = WindowPlan(image, roi, overlap)
    assert plan.starts == starts and plan.num_windows == count
    assert [(b, p - s - b) for b, p, s in zip(plan.pad_before, plan.padded, image)] == pads
    # enumeration order: first spatial axis slowest
    assert plan.windows == [(z, y, x) for z in starts[0] for y in starts[1] for x in starts[2]]
    # the restatement reads the table the same way
    rpads, rstarts, rwindows = R.window_starts(image, roi, overlap)
    assert rstarts == starts and rpads == pads and rwindows == plan.windows


def test_roi_entry_below_one_means_the_image_extent_and_2d():
    from medical_image_generation_amd.sliding import WindowPlan
    plan = WindowPlan((13, 18, 23), (0, 8, -1), 0.25)
    assert plan.roi == (13, 8, 23) and plan.starts == [[0], [0, 6, 10], [0]]
    plan = WindowPlan((18, 23), 8, (0.25, 0.5))
    assert plan.roi == (8, 8) and plan.starts == [[0, 6, 10], [0, 4, 8, 12, 15]]


@pytest.mark.parametrize("roi", [(8, 8, 16), (16,), (5, 7)])
@pytest.mark.parametrize("mode,sigma", [("constant", 0.125), ("gaussian", 0.125), ("gaussian", 0.05), ("gaussian", 0.3)])
def test_importance_map_matches_the_restatement(roi, mode, sigma):
    from medical_image_generation_amd.sliding import importance_map
    got = importance_map(roi, mode, sigma)
    want = R.importance(roi, mode, sigma).numpy()
    assert got.dtype == np.float64 and got.shape == tuple(roi)
    assert np.max(np.abs(got - want) / want) <= 2.0 ** -24  # equal to fp32 rounding


def test_gaussian_floor_is_active_for_a_narrow_sigma():
    from medical_image_generation_amd.sliding import importance_map
    m = importance_map((16,), "gaussian", 0.05)
    # sigma = 0.8 voxels: exp(-(7.5)^2 / 1.28) is far below the floor at the ends, the centre is not floored
    assert m[0] == 1e-3 and m[-1] == 1e-3 and m[7] == m[8] > 0.8
    assert (m == 1e-3).sum() == 10
    unfloored = np.exp(-((np.arange(16) - 7.5) ** 2) / (2 * 0.8 ** 2))
    assert np.allclose(m, np.maximum(unfloored, 1e-3), rtol=1e-15)
    assert importance_map((16,), "gaussian", 0.25).min() > 1e-3  # a wide one does not reach it: exp(-7.5^2 / 32) = 0.17


@pytest.mark.parametrize("factor", ["down4", "up4"])
def test_nearest_resample_of_the_importance_map(factor):
    from medical_image_generation_amd.sliding import importance_map, resample_nearest
    roi = (8, 16, 16)
    t = tuple(r // 4 for r in roi) if factor == "down4" else tuple(4 * r for r in roi)
    imp = importance_map(roi, "gaussian", 0.125)
    got = resample_nearest(imp, t)
    assert got.shape == t
    want = R.nearest(torch.from_numpy(imp), t).numpy()
    assert np.array_equal(got, want)
    if factor == "down4":
        assert np.array_equal(got, imp[::4, ::4, ::4])
    else:
        assert np.array_equal(got, imp.repeat(4, 0).repeat(4, 1).repeat(4, 2))


def test_output_extents_must_map_to_whole_voxels():
    from medical_image_generation_amd.sliding import WindowPlan
    plan = WindowPlan((16, 24, 32), (8, 16, 16), 0.5)  # starts 4 on axis 0
    assert plan.scaled((2, 4, 4)) == ((4, 6, 8), (0, 0, 0), (4, 6, 8))
    assert plan.scaled((32, 64, 64)) == ((64, 96, 128), (0, 0, 0), (64, 96, 128))
    with pytest.raises(ValueError, match="window start"):
        plan.scaled((1, 4, 4))  # start 4 * 1 / 8
    with pytest.raises(ValueError, match="padded image extent"):
        WindowPlan((13, 16, 16), (8, 16, 16), 0.0).scaled((2, 4, 4))  # 13 / 4
    padded = WindowPlan((5, 18, 24), (8, 8, 16), 0.5)  # pad 1 before: 1 / 4 of a latent voxel
    with pytest.raises(ValueError):
        padded.scaled((2, 2, 4))
    with pytest.raises(ValueError):
        plan.scaled((2, 4))


def test_filler_rows_appear_exactly_when_the_last_call_is_short():
    from medical_image_generation_amd.sliding import WindowPlan
    for image, roi, overlap, _, count, _ in TABLE:
        plan = WindowPlan(image, roi, overlap)
        for n in (1, 2, 3):
            for b in (1, 2, 3, 4, 5, 7):
                rows = plan.rows(n, b)
                fillers = int((rows[..., 0] < 0).sum())
                total = count * n
                assert rows.shape == (-(-total // b), b, 4)
                assert (fillers > 0) == (total % b != 0) and fillers == -total % b
                flat = rows.reshape(-1, 4)
                assert (flat[total:, 0] == -1).all() and (flat[total:, 1:] == 0).all()  # only at the end
                assert [tuple(r) for r in flat[:total]] == [(i,) + w for i in range(n) for w in plan.windows]
                want = R.batches(count, n, b)
                assert [[None if r[0] < 0 else int(r[0]) * count + plan.windows.index(tuple(r[1:])) for r in call] for call in rows] == want


def test_refusals_name_the_keyword():
    from medical_image_generation_amd.sliding import SlidingWindowInferer, sliding_window_inference
    with pytest.raises(NotImplementedError, match="circular"):
        SlidingWindowInferer(8, padding_mode="circular")
    for kw in ("roi_weight_map", "process_fn", "buffer_steps"):
        with pytest.raises(NotImplementedError, match=kw):
            SlidingWindowInferer(8, **{kw: 1})
        with pytest.raises(NotImplementedError, match=kw):
            sliding_window_inference(torch.zeros(1, 1, 8, 8, 8), 8, 1, lambda t: t, **{kw: 1})
    x = torch.zeros(1, 1, 8, 8, 8)
    for kw in ("sw_device", "device"):  # differs from the inputs' device (cpu)
        with pytest.raises(NotImplementedError, match=kw):
            SlidingWindowInferer(8, **{kw: "cuda"})(x, lambda t: t)
        with pytest.raises(NotImplementedError, match=kw):
            sliding_window_inference(x, 8, 1, lambda t: t, **{kw: "cuda"})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SlidingWindowInferer(8, device="cpu")(x, lambda t: t)  # same device, but the product has no CPU path
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SlidingWindowInferer(8)(x, lambda t: t)
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="overlap"):
            SlidingWindowInferer(8, overlap=bad)
    with pytest.raises(ValueError):
        SlidingWindowInferer(8, mode="linear")
    with pytest.raises(ValueError):
        SlidingWindowInferer(8, padding_mode="wrap")
    with pytest.raises(ValueError):
        SlidingWindowInferer(8, sw_batch_size=0)


def test_decode_inferer_keyword_is_on_the_latent_inferer_surface():
    import inspect
    from medical_image_generation_amd.inferer import LatentDiffusionInferer
    for name in ("sample", "img2img", "inpaint"):
        p = inspect.signature(getattr(LatentDiffusionInferer, name)).parameters
        assert "decode_inferer" in p and p["decode_inferer"].default is None
