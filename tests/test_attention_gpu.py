"""Fused attention kernels (csrc/attention.hip) against a plain PyTorch fp32 reference of softmax(QK^T*scale)V + residual,
forward and backward, through the C ABI.  bf16 operands, fp32 softmax: |err| <= 2e-2 of the reference's max."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = torch.device("cuda")


# One wide head (csrc/attention_wide.hip): the reference's latent UNets (configuration.py:894, num_head_channels = [0, 512, 768]) at
# the token counts of 8^3 .. 20^3 latents, a ragged count (1000, 125, 27), two images, and 8 tokens (fewer than one tile)
WIDE = [(1, 1, 512, 512), (2, 1, 1000, 512), (1, 1, 4096, 512), (1, 1, 8000, 512), (1, 1, 125, 512), (1, 1, 1000, 768), (2, 1, 27, 768),
        (1, 1, 8, 768)]


@pytest.mark.parametrize("B,H,S,d", [(1, 1, 64, 32), (2, 2, 64, 32), (1, 4, 512, 64), (2, 1, 1000, 64), (1, 2, 4096, 64), (1, 3, 200, 32)] + WIDE)
@pytest.mark.parametrize("split", [True, False])
def test_flash_attention_fwd_bwd(B, H, S, d, split):
    """split: hand the kernels their scratch, so the reduction axis is cut into up to 8 partial passes + a merge kernel
    (2 / 4 / 8 ways for the S = 512 / 1000 / 4096 cases); without it the single-pass kernels run."""
    from medical_image_generation_amd._lib import call, call_raw, ptr
    C = H * d
    g = torch.Generator().manual_seed(S + d)
    qkv = (torch.randn(B, S, 3 * C, generator=g) * 1.5).bfloat16()
    x = torch.randn(B, S, C, generator=g).bfloat16()
    dy = torch.randn(B, S, C, generator=g).bfloat16()
    scale = 1 / math.sqrt(d)
    # reference (fp32 on the bf16-rounded operands)
    qr = qkv.float().clone().requires_grad_(True)
    q, k, v = (qr[..., i * C:(i + 1) * C].reshape(B, S, H, d).permute(0, 2, 1, 3) for i in range(3))
    att = torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1)
    o = (att @ v).permute(0, 2, 1, 3).reshape(B, S, C)
    y_ref = o + x.float()
    o.backward(dy.float())
    # HIP
    qd, xd, dyd = qkv.to(dev).reshape(B * S, 3 * C), x.to(dev), dy.to(dev)
    y = torch.empty_like(xd)
    lse = torch.empty(B * H, S, device=dev)
    nws = call_raw("mi_attn_workspace_bytes", C, H, B, S) if split else 0
    assert call_raw("mi_attn_supported", C, H) == 1
    assert nws > 0 or not split or S < 512
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=dev)
    call("mi_attn_fwd", ptr(qd), 3 * C, C, H, B, S, scale, ptr(xd), ptr(y), ptr(lse), ptr(ws) if split else None, nws)
    err = float((y.float().cpu() - y_ref.detach()).abs().max())
    assert err <= 2e-2 * float(y_ref.abs().max()), f"fwd err {err}"
    lse_ref = torch.logsumexp((q @ k.transpose(-1, -2) * scale).detach(), dim=-1).reshape(B * H, S) / math.log(2)
    assert float((lse.cpu() - lse_ref).abs().max()) <= 2e-2
    dqkv = torch.zeros_like(qd)
    dsum = torch.empty(B * H, S, device=dev)
    call("mi_attn_bwd", ptr(qd), 3 * C, C, H, B, S, scale, ptr(y), ptr(xd), ptr(dyd), ptr(lse), ptr(dsum), ptr(dqkv),
         ptr(ws) if split else None, nws)
    ref = qr.grad.reshape(B * S, 3 * C)
    got = dqkv.float().cpu()
    for name, sl in (("dQ", slice(0, C)), ("dK", slice(C, 2 * C)), ("dV", slice(2 * C, 3 * C))):
        e = float((got[:, sl] - ref[:, sl]).abs().max())
        assert e <= 2.5e-2 * float(ref[:, sl].abs().max()), f"{name} err {e} vs {float(ref[:, sl].abs().max())}"


# ---------------------------------------------------------------------------------------------------------------------------------
# Per-element checks against the fp64 restatement in tests/attn_ref.py, at the smallest shapes where each path of the kernels exists
# (attn_ref.CASES: one row past a tile, one tile short of a split, a last split whose last tile holds one row, B * H > 1 under a split,
# every split count), on inputs that move the running max at every tile, on near-one-hot and on uniform attention.  Every output and
# the scratch start as NaN and are fenced by sentinel rows, so a row a kernel forgets, or one it writes too many, shows.
import functools  # noqa: E402
import json  # noqa: E402

from tests import attn_ref as R  # noqa: E402

SENT = 0x5A3C           # int16 pattern of the fence rows and of the gap columns of a pitched buffer
NAN16 = 0x7FC0          # bf16 NaN; two of them read as an fp32 NaN


def _cid(c):
    return "d%d-B%d-H%d-S%d-ns%d" % c


def _fenced(rows, cols, dtype):
    """[rows + 64, cols]: NaN where the kernel must write, 64 spare rows of the sentinel pattern behind"""
    t = torch.full((rows + 64, cols), math.nan, dtype=dtype, device=dev)
    t.view(torch.int16)[rows:] = SENT
    return t


def _fence_intact(t, rows):
    return bool((t.view(torch.int16)[rows:] == SENT).all())


@functools.lru_cache(maxsize=None)
def _reference(kind, case, resid):
    d, B, H, S, _ = case
    qkv, x, dy, scale = R.make_inputs(kind, B, H, S, d, resid=resid)
    return qkv, x, dy, scale, R.reference(qkv, x, dy, B, H, S, d, scale)


@functools.lru_cache(maxsize=None)
def _gpu(kind, case, ws=True, pitch=0, resid=True, want_lse=True):
    """Forward and backward through the C ABI on fenced, NaN-filled buffers; outputs as fp64 CPU tensors.  pitch: extra elements per row
    of qkv and dqkv (ld = 3C + pitch) with the base pointers advanced by as many, so the gap is the first `pitch` columns of a row."""
    from medical_image_generation_amd._lib import call, call_raw, ptr
    d, B, H, S, ns = case
    C, rows, ld = H * d, B * S, 3 * H * d + pitch
    qkv, x, dy, scale, _ = _reference(kind, case, resid)
    assert call_raw("mi_attn_supported", C, H) == 1
    nws = call_raw("mi_attn_workspace_bytes", C, H, B, S)
    assert nws == (ns * B * S * 6 * C if ns > 1 else 0), f"split count of {case}: scratch of {nws} bytes"
    qd = torch.full((rows, ld), math.nan, dtype=torch.bfloat16, device=dev)  # a read of a gap column poisons the result
    qd[:, pitch:] = qkv.reshape(rows, 3 * C).to(dev)
    xd, dyd = (x.to(dev).contiguous() if resid else None), dy.to(dev).contiguous()
    wsb = torch.full((nws // 2 + 2048,), NAN16, dtype=torch.int16, device=dev)
    wsb[nws // 2:] = SENT
    wp, wn = (ptr(wsb), nws) if ws else (None, 0)

    def fwd(with_lse):
        y, lse = _fenced(rows, C, torch.bfloat16), _fenced(B * H * S, 1, torch.float32)
        call("mi_attn_fwd", qd.data_ptr() + 2 * pitch, ld, C, H, B, S, scale, ptr(xd), ptr(y), ptr(lse) if with_lse else None, wp, wn)
        torch.cuda.synchronize()
        assert _fence_intact(y, rows) and _fence_intact(lse, B * H * S) and _fence_intact(wsb, nws // 2), "forward wrote past its rows"
        return y, lse

    y, lse = fwd(True)
    if not want_lse:  # lse = NULL: the same output, bit for bit, and lse untouched
        y0, lse0 = fwd(False)
        assert torch.equal(y0.view(torch.int16), y.view(torch.int16))
        assert bool(torch.isnan(lse0[:B * H * S]).all())
    wsb[:nws // 2] = NAN16
    dqkv, dsum = _fenced(rows, ld, torch.bfloat16), _fenced(B * H * S, 1, torch.float32)
    dqkv.view(torch.int16)[:rows, :pitch] = SENT
    call("mi_attn_bwd", qd.data_ptr() + 2 * pitch, ld, C, H, B, S, scale, ptr(y), ptr(xd), ptr(dyd), ptr(lse), ptr(dsum),
         dqkv.data_ptr() + 2 * pitch, wp, wn)
    torch.cuda.synchronize()
    assert _fence_intact(dqkv, rows) and _fence_intact(dsum, B * H * S) and _fence_intact(wsb, nws // 2), "backward wrote past its rows"
    assert bool((dqkv.view(torch.int16)[:rows, :pitch] == SENT).all()), "backward wrote into the gap columns"
    g = dqkv[:rows, pitch:].double().cpu()
    return dict(y=y[:rows].double().cpu().reshape(B, S, C), lse=lse[:B * H * S, 0].double().cpu().reshape(B * H, S),
                dsum=dsum[:B * H * S, 0].double().cpu().reshape(B * H, S),
                dQ=g[:, :C].reshape(B, S, C), dK=g[:, C:2 * C].reshape(B, S, C), dV=g[:, 2 * C:].reshape(B, S, C))


def _check(kind, case, ws, tag="", **kw):
    d, B, H, S, ns = case
    qkv, x, _, _, ref = _reference(kind, case, kw.get("resid", True))
    got = _gpu(kind, case, ws, **kw)
    r = R.ratios(got, ref)
    print("ATTN", json.dumps(dict(d=d, split=bool(ws and ns > 1), kind=kind + tag, B=B, H=H, S=S, **{k: round(v, 4) for k, v in r.items()})))
    assert all(v <= 1.0 for v in r.values()), f"err / bound per quantity: {r}"
    if kind == "qzero":
        assert R.qzero_failed(got, qkv, x, B, H, S, d) == []


def _ws_modes(cases):  # with the scratch always; without it where that changes the path
    return [pytest.param(c, w, id=_cid(c) + ("-ws" if w else "-nows")) for c in cases for w in ((True, False) if c[4] > 1 else (True,))]


@pytest.mark.parametrize("case,ws", _ws_modes(R.CASES))
def test_attention_elementwise_gaussian(case, ws):
    _check("gauss", case, ws)


@pytest.mark.parametrize("case,ws", _ws_modes(R.KIND_CASES))
@pytest.mark.parametrize("kind", R.KINDS[1:])
def test_attention_elementwise_hard_inputs(kind, case, ws):
    """rising: the running max moves at every tile and the early splits' merge weights vanish; onehot: amplitude 6; qzero: uniform
    attention, lse = log2(S) to 1e-5 on every row."""
    _check(kind, case, ws)


ARG_CASES = [(32, 2, 2, 65, 1), (64, 2, 2, 520, 2), (32, 2, 2, 1000, 4), (512, 1, 1, 65, 1), (512, 2, 1, 513, 2), (768, 1, 1, 513, 2)]


@pytest.mark.parametrize("case,ws", _ws_modes(ARG_CASES))
@pytest.mark.parametrize("variant", ["pitch", "noresid", "nolse", "pitch-noresid"])
def test_attention_arguments(variant, case, ws):
    """ld = 3C + 8 on channel slices of wider qkv / dqkv buffers, resid = NULL forward and backward, lse = NULL in the forward."""
    kw = dict(pitch=8 if "pitch" in variant else 0, resid="noresid" not in variant, want_lse=variant != "nolse")
    _check("gauss", case, ws, tag="/" + variant, **kw)


@pytest.mark.parametrize("case", [c for c in R.CASES if c[4] > 1], ids=_cid)
@pytest.mark.parametrize("kind", ["gauss", "rising"])
def test_attention_split_matches_single_pass(kind, case):
    """A split run differs from the single pass on the same data by the partial outputs' rounding, the two runs' own P roundings (against
    different running maxima) and their output roundings -- attn_ref.split_bound -- and in lse by 1e-5."""
    _, _, _, _, ref = _reference(kind, case, True)
    a, b = _gpu(kind, case, True), _gpu(kind, case, False)
    dy = (a["y"] - b["y"]).abs()
    r = float((dy / R.split_bound(ref)).max())
    dl = float((a["lse"] - b["lse"]).abs().max())
    print("ATTN-SPLIT", json.dumps(dict(d=case[0], kind=kind, S=case[3], y=round(r, 4), lse=dl)))
    assert r <= 1.0 and dl <= 1e-5, (r, dl)
