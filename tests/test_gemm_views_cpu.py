"""The view wrappers of the NT GEMM and the transpose (hipops.gemm_nt / transpose) check what the kernels require BEFORE any library
call: a stride mistake there reads out of bounds on the GPU.  No GPU: the library call is patched out."""
import pytest
import torch

from medical_image_generation_amd import hipops

BF16 = torch.bfloat16


def _bf(*shape):
    return torch.zeros(shape, dtype=BF16)


@pytest.fixture
def no_call(monkeypatch):
    def fail(name, *args):
        pytest.fail(f"{name} was reached with arguments the wrapper must refuse")

    monkeypatch.setattr(hipops, "call", fail)


def test_gemm_nt_refuses_what_the_kernel_cannot_take(no_call):
    a, b = _bf(2, 3, 5, 16), _bf(2, 3, 7, 16)
    with pytest.raises(ValueError, match="last-dim stride"):
        hipops.gemm_nt(_bf(2, 3, 5, 32)[..., ::2], b)                       # K axis strided
    with pytest.raises(ValueError, match="last-dim stride"):
        hipops.gemm_nt(a, b, out=torch.zeros(2, 3, 5, 14)[..., ::2])
    with pytest.raises(ValueError, match="multiple of 8"):
        hipops.gemm_nt(_bf(5, 12), _bf(7, 12))
    with pytest.raises(ValueError, match="multiple of 8"):
        hipops.gemm_nt(_bf(5, 16), _bf(7, 24))                              # K differs
    with pytest.raises(ValueError, match="batch shape"):
        hipops.gemm_nt(a, _bf(2, 4, 7, 16))                                 # heads 3 vs 4
    with pytest.raises(ValueError, match="batch shape"):
        hipops.gemm_nt(a, b, out=torch.zeros(3, 5, 7))                      # the output cannot broadcast
    with pytest.raises(ValueError, match="batch shape"):
        hipops.gemm_nt(a, b, res=_bf(2, 2, 5, 7))
    with pytest.raises(ValueError, match="two batch levels"):
        hipops.gemm_nt(_bf(2, 2, 3, 5, 16), _bf(2, 2, 3, 7, 16))
    with pytest.raises(ValueError, match="16-byte"):
        hipops.gemm_nt(_bf(5, 24)[:, 4:20], _bf(7, 16))                     # rows start 8 bytes off
    with pytest.raises(ValueError, match="16-byte"):
        hipops.gemm_nt(_bf(5, 20)[:, :16], _bf(7, 16))                      # 40-byte row pitch
    with pytest.raises(ValueError, match=r"expected \[.., 5, 7\]"):
        hipops.gemm_nt(a, b, res=_bf(2, 3, 5, 8))
    with pytest.raises(ValueError, match="accumulate adds into an fp32 out"):
        hipops.gemm_nt(a, b, out=_bf(2, 3, 5, 7), accumulate=True)


def test_transpose_refuses_what_the_kernel_cannot_take(no_call):
    with pytest.raises(ValueError, match="last-dim stride"):
        hipops.transpose(_bf(3, 5, 32)[..., ::2])
    with pytest.raises(ValueError, match="two batch levels"):
        hipops.transpose(_bf(2, 2, 3, 5, 16))
    with pytest.raises(ValueError, match="batch shape"):
        hipops.transpose(_bf(2, 3, 5, 16), pad_to=8, out=_bf(3, 16, 8))
    with pytest.raises(ValueError, match=r"expected bf16 \[.., 16, 8\]"):
        hipops.transpose(_bf(2, 3, 5, 16), pad_to=8, out=_bf(2, 3, 16, 5))
    with pytest.raises(AssertionError):
        hipops.transpose(_bf(5, 16), pad_to=16)
    # k_transpose zero-fills columns R .. min(R rounded up to 8, pitch): with R % 8 != 0 and a wider pitch they are a neighbour's
    for out in (_bf(16, 40)[:, :5], _bf(16, 8)[:, :5], _bf(2, 3, 16, 6)[..., :5], _bf(1, 40)[:, :5]):
        with pytest.raises(ValueError, match="row pitch"):
            hipops.transpose(_bf(*out.shape[:-2], 5, out.shape[-2]), out=out)
    with pytest.raises(ValueError, match="row pitch"):
        hipops.transpose(_bf(13, 16), out=_bf(16, 15)[:, 2:])                # the first 2 columns of the NEXT row would be zeroed


def test_transpose_takes_every_view_its_zero_fill_stays_inside(monkeypatch):
    """... and nothing else is refused: a dense ragged output (pitch R), a wider pitch with R % 8 == 0, and any pitch with pad_to=8."""
    calls = []
    monkeypatch.setattr(hipops, "call", lambda name, *args: calls.append((name,) + args))
    monkeypatch.setattr(hipops, "ptr", lambda t: None if t is None else t.data_ptr())
    hipops.transpose(_bf(5, 16))
    assert calls.pop()[5:9] == (_ANY, 5, 0, 0)
    hipops.transpose(_bf(2, 5, 16), out=_bf(2, 16, 5))
    assert calls.pop()[6:8] == (5, 80)
    hipops.transpose(_bf(8, 16), out=_bf(16, 40)[:, 32:])
    assert calls.pop()[6] == 40
    hipops.transpose(_bf(5, 16), pad_to=8, out=_bf(16, 40)[:, :8])
    assert calls.pop()[6] == 40
    hipops.transpose(_bf(2, 3, 27, 16), pad_to=8, out=_bf(2, 3, 16, 64)[..., 32:])
    assert calls.pop()[6:11] == (64, 3 * 16 * 64, 16 * 64, 27, 16)
    assert not calls


def test_views_reach_the_library_with_their_own_strides(monkeypatch):
    """Head views of a fused [B, S, 3 * heads * hd] matrix: pitch and both batch strides are the views' (z = B * heads, z2 = heads); an
    operand without batch dims broadcasts with stride 0; padded() widens a softmax result to its pitch."""
    calls = []
    monkeypatch.setattr(hipops, "call", lambda name, *args: calls.append((name,) + args))
    monkeypatch.setattr(hipops, "ptr", lambda t: None if t is None else t.data_ptr())
    B, S, S2, H, hd = 2, 5, 7, 3, 16
    c3 = 3 * H * hd
    wide, wide2 = _bf(B, S, c3), _bf(B, S2, c3)
    q = wide.view(B, S, 3, H, hd)[:, :, 0].permute(0, 2, 1, 3)
    k = wide2.view(B, S2, 3, H, hd)[:, :, 1].permute(0, 2, 1, 3)
    out = hipops.gemm_nt(q, k, alpha=0.25, out_f32=True)
    assert out.shape == (B, H, S, S2)
    assert calls.pop() == ("mi_gemm_nt_bf16", wide.data_ptr(), c3, S * c3, hd, wide2.data_ptr() + 2 * H * hd, c3, S2 * c3, hd,
                           out.data_ptr(), S2, H * S * S2, S * S2, None, None, 0, 0, 0, S, S2, hd, B * H, H, 0.25, 1, 0)
    probs = _bf(B, H, S, 8)[..., :S2]                                        # as softmax_fwd(pad8=True) returns it
    assert hipops.padded(probs).shape == (B, H, S, 8) and hipops.padded(probs).stride() == probs.stride()
    vt = hipops.transpose(wide2.view(B, S2, 3, H, hd)[:, :, 2].permute(0, 2, 1, 3), pad_to=8)
    assert vt.shape == (B, H, hd, 8)
    assert calls.pop() == ("mi_transpose_bf16", wide2.data_ptr() + 4 * H * hd, c3, S2 * c3, hd, vt.data_ptr(), 8, H * hd * 8, hd * 8, S2, hd, B * H, H)
    y, x = _bf(B, S, H * hd), _bf(B, S, H * hd)
    heads = lambda t: t.view(B, S, H, hd).permute(0, 2, 1, 3)  # noqa: E731
    hipops.gemm_nt(hipops.padded(probs), vt, out=heads(y), res=heads(x))
    assert calls.pop()[9:22] == (y.data_ptr(), H * hd, S * H * hd, hd, None, x.data_ptr(), H * hd, S * H * hd, hd, S, hd, 8, B * H)
    w = _bf(24, 16)
    o = hipops.gemm_nt(_bf(4, 5, 16), w, bias=None)                          # one batch level, shared weight
    assert o.shape == (4, 5, 24)
    assert calls.pop()[1:13] == (_ANY, 16, 80, 0, w.data_ptr(), 16, 0, 0, o.data_ptr(), 24, 120, 0)
    o2 = hipops.gemm_nt(_bf(5, 16), w)                                       # no batch: z = z2 = 1, strides 0
    assert calls.pop()[1:] == (_ANY, 16, 0, 0, w.data_ptr(), 16, 0, 0, o2.data_ptr(), 24, 0, 0, None, None, 0, 0, 0, 5, 24, 16, 1, 1, 1.0, 0, 0)
    assert not calls


class _Any:
    def __eq__(self, other):
        return True


_ANY = _Any()
