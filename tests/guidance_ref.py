"""fp64 restatement of classifier-free guidance (Ho & Salimans 2022; not part of the reference: PARITY UNPINNED) for the tests of
the guided `mi_diffusion_step` and of the guided sample loop.  TEST INFRASTRUCTURE: written from the formula alone,
on the oracle's fp32 U-Net and the fp64 DDIM rows of tests/ddim_ref.py; it does not import the product.

    m = m_uncond + w (m_cond - m_uncond)            w = 1: the conditional model, w = 0: the unconditional one

The unconditional branch runs the same net on the NULL condition: zero cross-attention context, zero concatenated condition channels,
and the label `null_class` for a class-conditional net.

The three routes, at the shapes the oracle finishes in seconds:
    class   unet2d_class, labels (1, 3), null_class 0
    xattn   unet2d_xattn, context [2, 5, 16]
    concat  unet_ldm rebuilt with in_channels=9, out_channels=8, one binary label channel
"""
import functools

import torch

from oracle import cases, nets, synth
from tests import ddim_ref

S = cases.SEED
GENTLE = dict(schedule="linear_beta", beta_start=1e-4, beta_end=2e-3)  # tests/test_ddim_gpu.py's loop schedule, for its stated reason
BOUND = 3e-2   # tests/test_ddim_gpu.py: the rel-L2 drift budget of an UNGUIDED bf16 loop over a few steps
STEPS = 4
# The scale of each route's loop tests: the smallest of 2, 2.5, 3, ... at which the guided oracle loop ends more than 5 * BOUND away
# from the conditional-only loop (tests/test_guidance_cpu.py verifies it), so that a wrong branch order, or a dropped branch, cannot
# pass -- and no larger, because guidance multiplies the forward's rounding error by about |1 - w| + |w|.  Measured separations at
# w = 2: class 0.057 (too close: the labels move this small net little; 0.139 at 3.5, 0.167 at 4), xattn 0.256, concat 0.162.
W = {"class": 4.0, "xattn": 2.0, "concat": 2.0}
NULL_CLASS = 0
ROUTES = ("class", "xattn", "concat")


def combine(m_cond, m_uncond, w):
    """fp64 m_uncond + w (m_cond - m_uncond)."""
    mc, mu = m_cond.double(), m_uncond.double()
    return mu + float(w) * (mc - mu)


@functools.lru_cache(maxsize=None)
def case(route):
    """-> (kwargs of the net, its state dict, the oracle net in eval mode, sample shape, the conditioning {labels | context | cond})."""
    if route == "class":
        c = cases.UNET_CASES["unet2d_class"]
        kw, shape, cond = dict(c["kwargs"]), c["shape"], dict(labels=torch.tensor(c["class_labels"]))
    elif route == "xattn":
        c = cases.UNET_CASES["unet2d_xattn"]
        kw, shape, cond = dict(c["kwargs"]), c["shape"], dict(context=synth.tensor(S, "context", c["context"]))
    elif route == "concat":
        kw = dict(cases.UNET_CASES["unet_ldm"]["kwargs"], in_channels=9, out_channels=8)
        shape = (2, 8, 8, 8, 8)
        cond = dict(cond=(synth.ellipsoid_volume(S, "label", (2, 1, 8, 8, 8)) > 0).float())
    else:
        raise ValueError(route)
    ref = nets.DiffusionModelUNet(**kw)
    sd = synth.state_dict({k: tuple(v.shape) for k, v in ref.state_dict().items()}, S)
    ref.load_state_dict(sd)
    return kw, sd, ref.eval(), tuple(shape), cond


def null_of(cond):
    """The null condition of the unconditional branch."""
    out = {}
    if "labels" in cond:
        out["labels"] = torch.full_like(cond["labels"], NULL_CLASS)
    if "context" in cond:
        out["context"] = torch.zeros_like(cond["context"])
    if "cond" in cond:
        out["cond"] = torch.zeros_like(cond["cond"])
    return out


def forward(ref, x, t, cond):
    inp = torch.cat([x, cond["cond"]], dim=1) if "cond" in cond else x
    return ref(inp, torch.full((x.shape[0],), t, dtype=torch.int64), context=cond.get("context"), class_labels=cond.get("labels"))


def loop(ref, x, cond, w=None, n=STEPS, reverse=False, round_bf16=False):
    """The eta-0 DDIM loop (or its inversion) on the oracle net, the update in fp64.  w None: one forward per step on `cond`;
    w a float: two forwards per step (cond, null_of(cond)) combined in fp64.  round_bf16: both model outputs are rounded to bf16 first
    -- what the guided kernel reads -- to measure how much of the forward's rounding the combination lets through."""
    acp, _ = ddim_ref.alphas_cumprod(1000, **GENTLE)
    ts = ddim_ref.timesteps(1000, n)
    rows = ddim_ref.rows(acp, n, 0.0, reverse=reverse)
    rnd = (lambda m: m.bfloat16().float()) if round_bf16 else (lambda m: m)
    with torch.no_grad():
        for i, t in enumerate(ts[::-1] if reverse else ts):
            m = rnd(forward(ref, x, t, cond))
            if w is not None:
                m = combine(m, rnd(forward(ref, x, t, null_of(cond))), w)
            x = ddim_ref.update(rows[i], x, m, None, clip_sample=True)[0].float()
    return x


def rel(got, want):
    return float((got.double() - want.double()).norm() / want.double().norm())


@functools.lru_cache(maxsize=None)
def start(route):
    return synth.tensor(S, "sample_noise", case(route)[3])


@functools.lru_cache(maxsize=None)
def wants(route):
    """The oracle loops the tests of one route compare against, computed once: conditional-only, guided at W[route], unconditional."""
    _, _, ref, _, cond = case(route)
    x = start(route)
    return dict(cond=loop(ref, x, cond), guided=loop(ref, x, cond, W[route]), uncond=loop(ref, x, null_of(cond)))


@functools.lru_cache(maxsize=None)
def drift(route):
    """rel-L2 between the guided oracle loop in fp32 and the same loop with both model outputs rounded to bf16."""
    _, _, ref, _, cond = case(route)
    return rel(loop(ref, start(route), cond, W[route], round_bf16=True), wants(route)["guided"])


def bound(route):
    """max(BOUND, 2 x drift): the factor 2 covers the bf16 activations inside the net, which rounding only the output does not."""
    return max(BOUND, 2.0 * drift(route))
