"""CPU side of classifier-free guidance (not part of the reference: PARITY UNPINNED): the library exports the new entry points, the
fp64 restatement (tests/guidance_ref.py) has the limits it claims, and the scales of the GPU loop tests separate a guided trajectory
from a conditional-only one -- so a wrong branch order or a dropped branch cannot pass there -- with the bound those tests use
measured here, not guessed."""
import ctypes
import re

import pytest
import torch

from oracle import cases, synth
from tests import abi_header
from tests import guidance_ref as G

NEW = ("mi_qsample_drop", "mi_select_labels", "mi_cast_bf16_drop")
FOLDED = ("mi_ddpm_step_guided", "mi_ddim_step_guided")  # the guided update is mi_diffusion_step with a non-NULL guidance (ABI 20)


def test_library_exports_the_guidance_entry_points():
    from medical_image_generation_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    hdr = abi_header.text()
    for name in NEW:
        assert hasattr(lib, name), name
        assert len(abi_header.params(name)) == len(_lib.signature(name)[1]), name  # the binding's argument list is the header's
    for name in FOLDED:
        assert not hasattr(lib, name) and name not in _lib.exported_symbols() and not re.search(r"\b%s\b" % name, hdr), name
    step = abi_header.params("mi_diffusion_step")
    assert "const float* guidance" in step and len(step) == len(_lib.signature("mi_diffusion_step")[1])
    assert len(_lib.signature("mi_qsample_drop")[1]) == len(_lib.signature("mi_qsample")[1]) + 1


def test_combine_limits():
    mc, mu = synth.tensor(cases.SEED, "g_mc", (2, 3, 7)), synth.tensor(cases.SEED, "g_mu", (2, 3, 7))
    assert torch.equal(G.combine(mc, mu, 1.0), mc.double())
    assert torch.equal(G.combine(mc, mu, 0.0), mu.double())
    assert torch.allclose(G.combine(mc, mu, 2.5), 2.5 * mc.double() - 1.5 * mu.double(), rtol=0, atol=1e-12)
    assert G.combine(mc, mu, 2.5).dtype == torch.float64


@pytest.mark.parametrize("route", G.ROUTES)
def test_guided_oracle_loop_is_far_from_the_conditional_one(route):
    """At the route's scale the guided loop ends more than 5 bounds from the conditional-only loop, and the unconditional loop (the
    w = 0 end, what the graph-reuse test compares with) is as far from it; the bf16 drift of the guided loop, which sets the bound of
    the GPU tests, is printed.  Measured: class (w = 4) separation 0.167, drift 4.6e-3; xattn (w = 2) 0.256, 1.5e-3; concat (w = 2)
    0.162, 1.8e-3 -- so 2 x drift stays below BOUND and every route's bound is BOUND = 3e-2."""
    want = G.wants(route)
    sep, sep0, drift, bound = G.rel(want["guided"], want["cond"]), G.rel(want["uncond"], want["cond"]), G.drift(route), G.bound(route)
    print(f"\n[{route} w={G.W[route]}] guided vs conditional {sep:.3e}, unconditional vs conditional {sep0:.3e}, bf16 drift {drift:.3e}, bound {bound:.3e}")
    assert bound >= G.BOUND and bound == max(G.BOUND, 2 * drift)
    assert sep > 5 * bound
    assert sep0 > bound  # the w = 0 replay cannot pass with the conditional labels
    # the w = 1 and w = 0 ends of the guided loop are the two single-branch loops
    _, _, ref, _, cond = G.case(route)
    assert G.rel(G.loop(ref, G.start(route), cond, 1.0), want["cond"]) < 1e-5
    assert G.rel(G.loop(ref, G.start(route), cond, 0.0), want["uncond"]) < 1e-5


def test_draw_drop_refuses_a_bad_probability():
    from medical_image_generation_amd.trainer import draw_drop
    with pytest.raises(ValueError):
        draw_drop(4, 1.5, device="cpu")
    m = draw_drop(64, 0.25, generator=torch.Generator().manual_seed(3), device="cpu")
    assert m.dtype == torch.bool and m.shape == (64,) and 0 < int(m.sum()) < 64
    assert not draw_drop(8, 0.0, device="cpu").any() and draw_drop(8, 1.0, device="cpu").all()
