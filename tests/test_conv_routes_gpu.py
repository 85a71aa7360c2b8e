"""The routes behind the phase kernels (convph.hip).  Every Upsample + conv and every all-axes k3 s2 conv of the other tests runs on the
phase kernels, so the glue behind them is never reached there: the P->up fallback of mi_conv_fwd / mi_conv_dgrad / mi_conv_wgrad (nearest
upsample into d_xup, then the inner k3 s1 plan on the fine grid) and the space-to-depth forward / data gradient / weight gradient of an
all-axes k3 s2 conv (its weight gradient is otherwise served by the in-place class gather).  MI_CONVPH=0 switches the phase kernels off;
the library reads the knob once, so the cases run in a fresh child process.  Same fp32 torch references, same measure and same 1e-2 bound
as test_upsample_conv_fwd_dgrad_wgrad and test_conv_fwd_dgrad_wgrad (the child imports their helpers)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import math, sys
sys.path.insert(0, %r)
import torch
import torch.nn.functional as F
from medical_image_generation_amd import hipops as ops
from tests.test_kernels_gpu import rnd, cl, cf, check, dev

def run(plan, n, cin, cout, dims, ref_fwd, what):
    x = rnd(n, cin, *dims)
    w = rnd(cout, cin, 3, 3, 3, scale=1.0 / math.sqrt(cin * 27))
    bias = rnd(cout, seed=3)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = ref_fwd(xr, wr, bias)
    g = rnd(*y.shape, seed=4)
    y.backward(g)
    assert plan.out_dims == tuple(y.shape[2:])
    plan.pack(w.to(dev))
    xc, gc = cl(x), cl(g)
    check(cf(plan.fwd(xc, addvec=bias.to(dev))), y.detach(), 1e-2, what + " fwd")
    check(cf(plan.dgrad(gc)), xr.grad, 1e-2, what + " dgrad")
    dw = torch.ones_like(w).to(dev)  # wgrad accumulates
    cb = torch.ones(cout, device=dev)
    plan.wgrad(xc, gc, dw, colsum=cb)
    check(dw.cpu() - 1, wr.grad, 1e-2, what + " wgrad")
    check(cb.cpu() - 1, g.sum(dim=(0, 2, 3, 4)), 1e-2, what + " bias gradient")

for n, cin, cout, dims in [(1, 32, 32, (4, 8, 8)), (2, 64, 32, (3, 5, 7))]:
    run(ops.UpConvPlan(n, dims, cin, cout), n, cin, cout, dims,
        lambda x, w, b: F.conv3d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, b, padding=1), f"upconv fallback {cin}->{cout} {dims}")
for n, cin, cout, dims in [(1, 32, 32, (8, 8, 8)), (1, 64, 64, (6, 10, 12))]:
    run(ops.ConvPlan(n, dims, cin, cout, (3, 3, 3), (2, 2, 2), (1, 1, 1)), n, cin, cout, dims,
        lambda x, w, b: F.conv3d(x, w, b, stride=2, padding=1), f"k3 s2 by space-to-depth {cin}->{cout} {dims}")
torch.cuda.synchronize()
print("ROUTES OK")
"""


def test_routes_behind_the_phase_kernels():
    env = dict(os.environ, MI_CONVPH="0")
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ROUTES OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
