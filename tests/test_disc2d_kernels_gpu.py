"""Kernel-level parity of the 2-D k4 convolutions (csrc/disc2d.hip) against F.conv2d autograd in fp32 on the CPU, from the same
bf16-rounded input / weight / output gradient.  Budgets of the 3-D test_conv_gemm_layer: |err| <= 1e-2 * max|ref| for y, dx, dW and
the bias gradient; the forward is bf16 products summed in fp32 and rounded once, so every element of y is also within 2^-7 * max|y|.
Outputs and the split workspace are pre-filled with NaN (an element nobody writes shows), dW accumulates onto a random base, and the
weight gradient of two runs must be bit-identical (fixed-order fold, no float atomics)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

dev = torch.device("cuda")
BF16 = torch.bfloat16
BAD_ARG, UNSUPPORTED = 10001, 10002

# (N, Cin, Cout, H, W, stride)
MFMA_SHAPES = [
    (1, 16, 32, 2, 2, 2),        # one output pixel, 12 of the 16 taps are padding
    (2, 16, 32, 10, 14, 2),      # 70 rows: a ragged tile
    (1, 16, 32, 9, 13, 2),       # odd extents: the parity classes of the data gradient differ in rows
    (2, 128, 256, 3, 3, 1),      # every window touches padding
    (1, 256, 512, 5, 7, 1),      # 24 rows, K = 4096
    (2, 64, 128, 24, 24, 2),     # several K slabs and N tiles
    (2, 64, 128, 128, 128, 2),   # planner-sized: several workgroups and pixel splits
    (2, 256, 512, 32, 32, 1),    # 961 rows per image
]
EDGE_SHAPES = [(2, 1, 64, 32, 32, 2), (1, 2, 64, 40, 56, 2), (1, 1, 16, 7, 9, 2), (2, 512, 1, 4, 6, 1), (1, 128, 1, 3, 3, 1),
               (1, 16, 64, 6, 10, 2)]  # (the last: 16384 weights, above what the edge kernels keep in LDS -- they read the torch tensor)


def check(got, ref, tol, what):
    scale = float(ref.abs().max()) + 1e-12
    err = float((got - ref).abs().max())
    print(f"  {what}: max err {err:.4g} vs scale {scale:.4g} ({err / scale:.2e})")
    assert math.isfinite(err) and err <= tol * scale, f"{what}: max err {err:.4g} vs scale {scale:.4g}"


def nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def reference(shape, bias):
    n, cin, cout, h, w, s = shape
    torch.set_num_threads(16)
    g = torch.Generator().manual_seed(1000 * cin + cout + h * w + s)
    wt = (torch.randn(cout, cin, 4, 4, generator=g) / math.sqrt(cin * 16)).bfloat16().float()
    b = torch.randn(cout, generator=g) if bias else None
    x = torch.randn(n, cin, h, w, generator=g).bfloat16().float()
    xr, wr = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if bias else None
    yr = F.conv2d(xr, wr, br, stride=s, padding=1)
    gy = torch.randn(yr.shape, generator=g).bfloat16().float()
    yr.backward(gy)
    base = torch.randn(wt.shape, generator=g)  # what the arena gradient already holds: the kernels accumulate
    return dict(x=x, w=wt, b=b, gy=gy, y=yr.detach(), dx=xr.grad, dw=wr.grad, db=br.grad if bias else None, base=base)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(dev, BF16)


def compare(shape, r, y, dx, dw, db=None):
    n, cin, cout, h, w, s = shape
    yg = y.float().cpu().permute(0, 3, 1, 2)
    assert tuple(yg.shape) == tuple(r["y"].shape)
    check(yg, r["y"], 1e-2, "forward")
    assert float((yg - r["y"]).abs().max()) <= 2.0 ** -7 * float(r["y"].abs().max()), "forward: beyond one bf16 rounding"
    check(dx.float().cpu().permute(0, 3, 1, 2), r["dx"], 1e-2, "dx")
    check(dw.cpu() - r["base"], r["dw"], 1e-2, "dW")
    if db is not None:
        check(db.cpu() - 1.0, r["db"], 1e-2, "bias gradient")


@pytest.mark.parametrize("shape", MFMA_SHAPES, ids=lambda s: "n{}_{}to{}_{}x{}_s{}".format(*s))
def test_mfma_layer(shape):
    from medical_image_generation_amd._lib import call, call_raw, ptr
    n, cin, cout, h, w, s = shape
    r = reference(shape, False)
    ho, wo = r["y"].shape[2:]
    x, dy, wt = nhwc(r["x"]), nhwc(r["gy"]), r["w"].to(dev)
    wf, wd = nan((cout, 16 * cin), BF16), nan((16 * cin * cout,), BF16)
    call("mi_conv2d_k4_pack", ptr(wt), ptr(wf), ptr(wd), cin, cout, s)
    y, dx = nan((n, ho, wo, cout), BF16), nan((n, h, w, cin), BF16)
    dims = (n, h, w, cin, cout, s)
    call("mi_conv2d_k4_fwd", ptr(x), ptr(wf), ptr(y), *dims)
    call("mi_conv2d_k4_dgrad", ptr(dy), ptr(wd), ptr(dx), *dims)
    splits = call_raw("mi_conv2d_k4_wgrad_splits", *dims)
    assert splits >= 1
    dws = []
    for _ in range(2):
        dw = r["base"].to(dev)
        ws = nan((splits * 16 * cin * cout,), torch.float32)
        call("mi_conv2d_k4_wgrad", ptr(x), ptr(dy), ptr(dw), ptr(ws), *dims)
        dws.append(dw)
    torch.cuda.synchronize()
    print(f"\n[conv2d k4 MFMA {shape}] {splits} pixel splits")
    compare(shape, r, y, dx, dws[0])
    assert torch.equal(dws[0], dws[1]), "the weight gradient differs between two runs"


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "n{}_{}to{}_{}x{}_s{}".format(*s))
def test_edge_layer(shape):
    from medical_image_generation_amd._lib import call, call_raw, ptr
    n, cin, cout, h, w, s = shape
    r = reference(shape, True)
    ho, wo = r["y"].shape[2:]
    x, dy, wt, b = nhwc(r["x"]), nhwc(r["gy"]), r["w"].to(dev), r["b"].to(dev)
    y, dx = nan((n, ho, wo, cout), BF16), nan((n, h, w, cin), BF16)
    dims = (n, h, w, cin, cout, s)
    call("mi_conv2d_k4_edge_fwd", ptr(x), ptr(wt), ptr(b), ptr(y), *dims)
    call("mi_conv2d_k4_edge_dgrad", ptr(dy), ptr(wt), ptr(dx), *dims)
    splits = call_raw("mi_conv2d_k4_edge_wgrad_splits", *dims)
    assert splits >= 1
    dws = []
    for _ in range(2):
        dw, db = r["base"].to(dev), torch.ones(cout, device=dev)
        ws = nan((splits * (16 * cin * cout + cout),), torch.float32)
        call("mi_conv2d_k4_edge_wgrad", ptr(x), ptr(dy), ptr(dw), ptr(db), ptr(ws), *dims)
        dws.append((dw, db))
    torch.cuda.synchronize()
    print(f"\n[conv2d k4 edge {shape}] {splits} pixel splits")
    compare(shape, r, y, dx, dws[0][0], dws[0][1])
    assert torch.equal(dws[0][0], dws[1][0]) and torch.equal(dws[0][1], dws[1][1]), "the gradients differ between two runs"


def test_bad_arguments_are_refused_without_a_launch():
    from medical_image_generation_amd import _lib
    lib = _lib.load()
    t = torch.zeros(1 << 16, dtype=BF16, device=dev)
    f = torch.zeros(1 << 16, dtype=torch.float32, device=dev)
    p, q, st = t.data_ptr(), f.data_ptr(), None
    good = (1, 8, 8, 16, 32, 2)
    assert lib.mi_conv2d_k4_fwd(p, p, p, *good, st) == 0
    assert lib.mi_conv2d_k4_fwd(None, p, p, *good, st) == BAD_ARG and lib.mi_conv2d_k4_fwd(p, p, None, *good, st) == BAD_ARG
    assert lib.mi_conv2d_k4_dgrad(p, None, p, *good, st) == BAD_ARG
    assert lib.mi_conv2d_k4_wgrad(p, p, q, None, *good, st) == BAD_ARG
    assert lib.mi_conv2d_k4_pack(None, p, p, 16, 32, 2, st) == BAD_ARG and lib.mi_conv2d_k4_pack(q, p, p, 16, 32, 3, st) == BAD_ARG
    for fn in (lib.mi_conv2d_k4_fwd, lib.mi_conv2d_k4_dgrad):
        assert fn(p, p, p, 0, 8, 8, 16, 32, 2, st) == BAD_ARG      # no images
        assert fn(p, p, p, 1, 1, 8, 16, 32, 2, st) == BAD_ARG      # output extent below 1
        assert fn(p, p, p, 1, 8, 1, 16, 32, 1, st) == BAD_ARG
        assert fn(p, p, p, 1, 8, 8, 16, 32, 3, st) == BAD_ARG      # stride
        assert fn(p, p, p, 1, 8, 8, 8, 32, 2, st) == UNSUPPORTED   # channel counts outside the MFMA path
        assert fn(p, p, p, 1, 8, 8, 16, 16, 2, st) == UNSUPPORTED
        assert fn(p, p, p, 1, 8, 8, 16, 1, 1, st) == UNSUPPORTED
    assert lib.mi_conv2d_k4_wgrad(p, p, q, q, 1, 8, 8, 24, 32, 2, st) == UNSUPPORTED
    assert lib.mi_conv2d_k4_pack(q, p, p, 1, 64, 2, st) == UNSUPPORTED
    assert lib.mi_conv2d_k4_wgrad_splits(1, 8, 8, 8, 32, 2) == 0 and lib.mi_conv2d_k4_wgrad_splits(1, 1, 8, 16, 32, 2) == 0
    assert lib.mi_conv2d_k4_edge_fwd(p, None, None, p, 1, 8, 8, 1, 16, 2, st) == BAD_ARG
    assert lib.mi_conv2d_k4_edge_fwd(p, q, None, p, 1, 8, 8, 0, 16, 2, st) == BAD_ARG
    assert lib.mi_conv2d_k4_edge_dgrad(p, q, p, 1, 1, 1, 1, 16, 2, st) == BAD_ARG
    assert lib.mi_conv2d_k4_edge_wgrad(p, p, q, q, None, 1, 8, 8, 1, 16, 2, st) == BAD_ARG
    assert lib.mi_conv2d_k4_edge_wgrad_splits(1, 8, 1, 1, 16, 2) == 0
    torch.cuda.synchronize()
