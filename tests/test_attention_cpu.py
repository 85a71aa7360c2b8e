"""The attention tests' own instruments (tests/attn_ref.py), checked without a GPU: the bf16 rounding model of the kernels meets every
per-element bound at every shape and split count the GPU tests run, and each planted fault -- the defects a subtly wrong kernel would
have -- misses at least one.  No element is left out of any comparison."""
import math

import pytest
import torch

from tests import attn_ref as R


def _id(c):
    return "d%d-B%d-H%d-S%d-ns%d" % c


def _run(kind, case, nsplit, fault=None, resid=True):
    d, B, H, S, _ = case
    qkv, x, dy, scale = R.make_inputs(kind, B, H, S, d, resid=resid)
    ref = R.reference(qkv, x, dy, B, H, S, d, scale)
    got = R.rounding_model(qkv, x, dy, B, H, S, d, scale, nsplit, fault)
    return qkv, x, ref, got


@pytest.mark.parametrize("case", R.CASES, ids=_id)
def test_rounding_model_meets_every_bound(case):
    """Gaussian inputs, with and without the residual, at the expected split count and unsplit."""
    for resid in (True, False):
        for ns in sorted({1, case[4]}):
            _, _, ref, got = _run("gauss", case, ns, resid=resid)
            r = R.ratios(got, ref)
            assert all(v <= 1.0 for v in r.values()), (ns, resid, r)


@pytest.mark.parametrize("case", R.KIND_CASES, ids=_id)
@pytest.mark.parametrize("kind", R.KINDS[1:])
def test_rounding_model_meets_every_bound_on_hard_inputs(kind, case):
    d, B, H, S, _ = case
    for ns in sorted({1, case[4]}):
        qkv, x, ref, got = _run(kind, case, ns)
        r = R.ratios(got, ref)
        assert all(v <= 1.0 for v in r.values()), (ns, r)
        if kind == "qzero":
            assert R.qzero_failed(got, qkv, x, B, H, S, d) == []


@pytest.mark.parametrize("case", [c for c in R.CASES if c[4] > 1], ids=_id)
def test_rounding_model_split_against_single_pass(case):
    """The model's split and single-pass outputs sit within split_bound of each other, and not within the partial rounding alone."""
    d, B, H, S, ns = case
    qkv, x, dy, scale = R.make_inputs("gauss", B, H, S, d)
    ref = R.reference(qkv, x, dy, B, H, S, d, scale)
    a, b = R.rounding_model(qkv, x, dy, B, H, S, d, scale, ns), R.rounding_model(qkv, x, dy, B, H, S, d, scale, 1)
    delta = (a["y"] - b["y"]).abs()
    assert bool((delta <= R.split_bound(ref)).all())
    assert float((a["lse"] - b["lse"]).abs().max()) <= 1e-5
    assert not bool((delta <= R.U8 * ref["y"].abs() + R.U8 * ref["A"]).all())


def test_hard_inputs_are_hard():
    """The rising-max input moves the running max at every tile and starves the early splits; the near-one-hot input is one."""
    d, B, H, S = 32, 1, 1, 769
    qkv, x, dy, scale = R.make_inputs("rising", B, H, S, d)
    q, k, _ = R._split_qkv(qkv, B, H, S, d)
    t = (q @ k.transpose(-1, -2))[0, 0] * (scale * R.LOG2E)
    tile_max = torch.stack([t[:, a:a + 64].max(-1).values for a in range(0, S, 64)])
    assert bool((tile_max[1:-1] - tile_max[:-2] > 4).all()), "each full tile must raise every query's max by a large factor"
    assert bool((tile_max[-1] > tile_max[-2]).all()), "and so must the one-key last tile"
    assert 50 < float(t.max()) < 75 and -75 < float(t.min()) < -50
    m = [t[:, a:b].max(-1).values for a, b in R.split_ranges(S, d, 3)]
    assert float((m[2] - m[0]).min()) > 40, "the first split's merge weight must vanish against the last's"
    qkv, x, dy, scale = R.make_inputs("onehot", B, H, S, d)
    ref = R.reference(qkv, x, dy, B, H, S, d, scale)
    q, k, _ = R._split_qkv(qkv, B, H, S, d)
    P = torch.exp2((q @ k.transpose(-1, -2))[0, 0] * (scale * R.LOG2E) - ref["lse"][0][:, None])
    assert float(P.max(-1).values.median()) > 0.9


FAULT_CASES = [
    # fault, input kind, (d, B, H, S, nsplit), quantities of which at least one must fail
    ("pad_unmasked", "gauss", (32, 1, 3, 200, 1), ("y",)),
    ("pad_unmasked", "gauss", (32, 1, 3, 200, 1), ("lse",)),
    ("pad_unmasked", "gauss", (32, 2, 2, 1000, 4), ("lse",)),
    ("pad_unmasked", "gauss", (64, 2, 1, 1000, 4), ("lse",)),
    ("pad_unmasked", "gauss", (512, 2, 1, 1000, 4), ("lse",)),
    ("key_dropped", "gauss", (64, 1, 4, 512, 2), ("y", "lse")),
    ("key_dropped", "gauss", (512, 1, 1, 512, 2), ("y", "lse")),
    ("merge_wrong_max", "gauss", (32, 1, 1, 513, 2), ("y", "lse")),
    ("merge_wrong_max", "gauss", (64, 1, 1, 513, 2), ("y", "lse")),
    ("merge_wrong_max", "gauss", (512, 1, 1, 513, 2), ("y", "lse")),
    ("dsum_from_y", "gauss", (32, 1, 1, 65, 1), ("dsum",)),
    ("dsum_from_y", "gauss", (512, 1, 1, 65, 1), ("dsum",)),
    ("row_unwritten", "gauss", (32, 2, 2, 65, 1), ("y",)),
    ("row_unwritten", "gauss", (32, 2, 2, 65, 1), ("dQ",)),
    ("row_unwritten", "gauss", (32, 2, 2, 65, 1), ("dK",)),
    ("row_unwritten", "gauss", (32, 2, 2, 65, 1), ("dV",)),
    ("row_unwritten_nan", "gauss", (64, 2, 2, 65, 1), ("y",)),
    ("row_unwritten_nan", "gauss", (64, 2, 2, 65, 1), ("dQ",)),
    ("row_unwritten_nan", "gauss", (512, 1, 1, 65, 1), ("dK",)),
    ("row_unwritten_nan", "gauss", (512, 1, 1, 65, 1), ("dV",)),
]


@pytest.mark.parametrize("fault,kind,case,names", FAULT_CASES, ids=lambda v: _id(v) if isinstance(v, tuple) and len(v) == 5 else None)
def test_planted_fault_misses_a_bound(fault, kind, case, names):
    _, _, ref, ok = _run(kind, case, case[4])
    assert R.failed(ok, ref) == [], "the fault-free model must pass where the fault is planted"
    _, _, ref, got = _run(kind, case, case[4], fault)
    assert R.failed(got, ref, names=names), (fault, R.ratios(got, ref))


@pytest.mark.parametrize("case", [(32, 2, 2, 1000, 4), (64, 2, 1, 1000, 4), (512, 2, 1, 1000, 4), (32, 1, 3, 200, 1)], ids=_id)
def test_unmasked_pad_keys_miss_the_uniform_attention_check(case):
    """At S = 1000 the 24 zero-score pad keys move a Gaussian input's output by about 2^-9 of itself -- one bf16 rounding, which the
    forward bound cannot tell; only lse of the rows with the smallest sums gives it away there (FAULT_CASES; the figures are printed
    here).  q = 0 makes the mask exact on every row: lse = log2(S) to 1e-5."""
    d, B, H, S, ns = case
    qkv, x, ref, ok = _run("qzero", case, ns)
    assert R.qzero_failed(ok, qkv, x, B, H, S, d) == [] and R.failed(ok, ref) == []
    _, _, _, got = _run("qzero", case, ns, "pad_unmasked")
    assert "lse" in R.qzero_failed(got, qkv, x, B, H, S, d)
    shift = abs(float(got["lse"][0, 0]) - math.log2(S))
    assert shift > 100 * 1e-5, shift
    _, _, gref, ggot = _run("gauss", case, ns, "pad_unmasked")
    print("Gaussian input, pad keys unmasked, err / bound:", case, R.ratios(ggot, gref))


def test_a_missing_number_fails():
    """The comparison treats NaN and inf as failures, never as 'not greater than the bound'."""
    case = (32, 1, 1, 33, 1)
    _, _, ref, got = _run("gauss", case, 1)
    for n in R.QUANTITIES:
        for bad in (math.nan, math.inf):
            g = {k: v.clone().contiguous() for k, v in got.items()}
            g[n].view(-1)[-1] = bad
            assert R.failed(g, ref) == [n]
