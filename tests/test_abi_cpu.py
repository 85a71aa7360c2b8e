"""CPU-side checks of the drop-in boundary: the C-ABI library builds/loads without a GPU and exports exactly the entry
points include/medimgen_hip.h declares; the host-side module mirrors the reference's constructor surface, state_dict
names and error behaviour; there is no CPU fallback (the product fails loudly off-GPU)."""
import ctypes as C
import os
import re

import pytest
import torch

from oracle import cases, nets
from tests import abi_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from medical_image_generation_amd import _lib
    lib = _lib.load()  # raises if the .so is missing
    # one statement of the version the loader checks: the source returns the header's macro, the header defines it once, the library has it
    api = open(os.path.join(ROOT, "medical_image_generation_amd", "csrc", "api.hip")).read()
    assert re.search(r"\bmi_abi_version\s*\(\s*void\s*\)\s*\{\s*return MI_ABI_VERSION;\s*\}", api)
    defined = re.findall(r"^[ \t]*#[ \t]*define[ \t]+MI_ABI_VERSION[ \t]+(\d+)", abi_header.text(), re.M)
    assert len(defined) == 1 and len(re.findall(r"\bdefine\s+MI_ABI_VERSION\b", abi_header.text())) == 1
    assert lib.mi_abi_version() == int(defined[0]) == _lib.ABI_VERSION
    declared = abi_header.names()
    assert declared == set(_lib.exported_symbols())
    for name in declared:
        assert hasattr(lib, name), name


def test_binding_takes_every_argument_list_from_the_header():
    """Argument counts by the tests' own comma split, for every entry point; the argtypes load() set on the library are the table's."""
    from medical_image_generation_amd import _lib
    lib = _lib.load()
    for name in sorted(abi_header.names()):
        restype, argtypes = _lib.signature(name)
        written = abi_header.params(name)
        assert len(written) == len(argtypes), name
        for p, t in zip(written, argtypes):  # a pointer in the text is a pointer in the binding, and nothing else is
            assert (t is C.c_void_p) == ("*" in p or p.endswith("]") or p.startswith("hipStream_t ")), (name, p)
        fn = getattr(lib, name)
        assert list(fn.argtypes) == argtypes and fn.restype is restype, name
    wide = {n for n in _lib.exported_symbols() if _lib.signature(n)[0] is C.c_int64}
    assert wide == {"mi_gn_workspace_bytes", "mi_attn_workspace_bytes", "mi_aug_stats_workspace_bytes", "mi_meter_bytes",
                    "mi_pp_stats_workspace_bytes", "mi_dm_gram_workspace_bytes"}
    assert all(_lib.signature(n)[0] is C.c_int for n in set(_lib.exported_symbols()) - wide)
    # by-value classes that load and run when they are wrong
    assert _lib.signature("mi_dm_finalize")[1][8:10] == [C.c_double, C.c_double] and _lib.signature("mi_dm_finalize")[1][5] is C.c_int64
    assert _lib.signature("mi_cast_f32_to_bf16")[1] == [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    assert _lib.signature("mi_avgpool_fwd")[1][7:9] == [C.c_void_p, C.c_void_p]  # const int kernel[3], const int stride[3]
    assert _lib.signature("mi_conv_pack_batch_create")[1] == [C.c_void_p] * 3 + [C.c_int]  # T**, T* const*, const T* const*


SYNTHETIC = """
/* block comment with call-like text: mi_fake(int a, int b); and (parentheses, commas) */
#ifndef SYNTHETIC_H
#define SYNTHETIC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define MI_ERR_BAD 10001
#define MI_REPLICAS 16 /* a trailing comment that runs
                        * over several lines: mi_other(int x); MI_REPLICAS * 2 */
#define MI_NOT_AN_INTEGER 1.5
// a line comment: int mi_line(int a);
typedef struct mi_plan mi_plan;
enum mi_kind {
  MI_K_NONE = 0,
  MI_K_A = 1, /* mi_k(1, 2) */
  MI_K_B = 7
};
enum { MI_OP_X = 0, MI_OP_Y = -2 };
int mi_version(void);
int mi_nothing();
int64_t mi_bytes(int N, int64_t V);
int mi_all(const void* a, mi_plan** out, mi_plan* const* plans, const int k[3], int64_t n, float f, double d, const float *const *w,
           const int count, hipStream_t stream);
int mi_split(const void* x,
             int n,
             hipStream_t stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_header_parser_maps_every_abi_class():
    from medical_image_generation_amd._lib import _parse_header
    p, i, l, f, d = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double
    functions, constants = _parse_header(SYNTHETIC)
    assert functions == {"mi_version": (i, []), "mi_nothing": (i, []), "mi_bytes": (l, [i, l]),
                         "mi_all": (i, [p, p, p, p, l, f, d, p, i, p]), "mi_split": (i, [p, i, p])}
    assert constants == {"MI_ERR_BAD": 10001, "MI_REPLICAS": 16, "MI_K_NONE": 0, "MI_K_A": 1, "MI_K_B": 7, "MI_OP_X": 0, "MI_OP_Y": -2}


@pytest.mark.parametrize("line,quoted", [
    ("int mi_bad(const void* x, size_t n);", "size_t n"),                    # an unknown parameter type
    ("int mi_bad(mi_plan plan, int n);", "mi_plan plan"),                     # a struct by value
    ("int mi_bad(struct mi_plan plan);", "struct mi_plan plan"),
    ("int mi_bad(unsigned int n);", "unsigned int n"),
    ("float mi_bad(int n);", "float mi_bad(int n);"),                         # a return type that is not a status or a byte count
    ("const void* mi_bad(int n);", "const void* mi_bad(int n);"),
    ("int mi_bad(int n,);", "int mi_bad(int n,);"),
    ("int mi_version(int again);", "int mi_version(int again);"),            # declared twice
    ("enum { MI_IMPLICIT, MI_NEXT = 2 };", "MI_IMPLICIT"),                    # only explicit enumerator values
    ("enum { MI_EXPR = 1 << 2 };", "MI_EXPR = 1 << 2"),
], ids=["size_t", "struct_by_value", "struct_keyword", "unsigned", "float_return", "pointer_return", "empty_parameter", "twice",
        "implicit_enumerator", "enumerator_expression"])
def test_header_parser_rejects_what_it_does_not_understand(line, quoted):
    from medical_image_generation_amd._lib import _parse_header
    with pytest.raises(RuntimeError, match=re.escape(quoted)):
        _parse_header(SYNTHETIC.replace("int mi_nothing();", "int mi_nothing();\n" + line))


def test_header_parser_constants_reach_the_public_names():
    """The product's public constants are the header's; the literals here pin the values independently."""
    from medical_image_generation_amd import _lib, augment, hipops, sliding, trainer
    c = _lib.constants()
    assert c is _lib.constants()  # parsed once
    assert (c["MI_ERR_BAD_ARG"], c["MI_ERR_UNSUPPORTED"]) == (10001, 10002) and sorted(_lib._ERRS) == [10001, 10002]
    assert "MI_ERR_BAD_ARG" in _lib._ERRS[10001] and "MI_ERR_UNSUPPORTED" in _lib._ERRS[10002]
    assert hipops.GN_FUSED_REPLICAS == c["MI_GN_FUSED_REPLICAS"] == 16
    assert trainer.METER_HEADER == c["MI_METER_HEADER"] == 4 and c["MI_METER_PARTIALS"] == 1024
    assert (augment.SCALE, augment.CONTRAST, augment.GAMMA, augment.RESTORE_STATS, augment.ADD_NOISE, augment.CLAMP01) == (0, 1, 2, 3, 4, 5)
    assert sliding.PAD_MODES == {"constant": 0, "reflect": 1, "replicate": 2}
    assert (c["MI_DM_FID"], c["MI_DM_MMD"], c["MI_DM_KID"]) == (0, 1, 2)
    assert c["MI_CK_1X1_STREAM"] == 17 and c["MI_CK_COUNT"] == 34


def test_load_refuses_a_missing_header_and_a_dead_nocheck_name(tmp_path, monkeypatch):
    from medical_image_generation_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "_NOCHECK", _lib._NOCHECK | {"mi_renamed_away"})
    with pytest.raises(RuntimeError, match="mi_renamed_away"):
        _lib.load()
    monkeypatch.undo()
    gone = str(tmp_path / "include" / "medimgen_hip.h")
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "HEADER_PATH", gone)
    _lib._header.cache_clear()
    try:
        with pytest.raises(RuntimeError, match=re.escape(gone)):
            _lib.load()
    finally:
        monkeypatch.undo()
        _lib._header.cache_clear()
    assert _lib.constants()["MI_ABI_VERSION"] == _lib.ABI_VERSION  # read again from the real header


def test_stale_library_is_refused(tmp_path, monkeypatch):
    """A library whose mi_abi_version() differs from the binding's (an old build left behind by a pull: *.so is not tracked) must not
    load -- several entry points changed their argument lists under unchanged names."""
    import subprocess
    from medical_image_generation_amd import _lib
    src = tmp_path / "stale.c"
    src.write_text(f"int mi_abi_version(void) {{ return {_lib.ABI_VERSION - 1}; }}\n")
    so = tmp_path / "libstale.so"
    subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    monkeypatch.setattr(_lib, "LIB_PATH", str(so))
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(RuntimeError, match="stale library"):
        _lib.load()


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "medical_image_generation_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), fn


@pytest.mark.parametrize("name", ["unet_c1", "unet3d", "unet_ldm"])
def test_unet_state_dict_names_match_reference(golden, name):
    from medical_image_generation_amd.unet import DiffusionModelUNet
    c = cases.UNET_CASES[name]
    net, ref = DiffusionModelUNet(**c["kwargs"]), nets.DiffusionModelUNet(**c["kwargs"])
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    _, meta = golden(name)  # names of the parameters that receive a gradient in the REFERENCE
    trainable = {n for n, _, t in net._entries if t}
    assert sorted(trainable) == meta["grad_names"].split("\n")
    # pristine init: zero_module'd tensors are zero, like the reference (UNet:649, 1934)
    sd = net.state_dict()
    assert float(sd["out.2.conv.weight"].abs().max()) == 0 and float(sd["down_blocks.0.resnets.0.conv2.conv.weight"].abs().max()) == 0


def test_unet_constructor_and_forward_errors():
    from medical_image_generation_amd.unet import DiffusionModelUNet
    with pytest.raises(ValueError):
        DiffusionModelUNet(3, 1, 1, num_channels=(30, 64), attention_levels=(False, False))
    with pytest.raises(ValueError):
        DiffusionModelUNet(3, 1, 1, num_channels=(32, 64), attention_levels=(False, False), cross_attention_dim=8)
    with pytest.raises(ValueError):
        DiffusionModelUNet(3, 1, 1, num_channels=(32, 64), attention_levels=(False, False), num_res_blocks=(1, 2, 3))
    net = DiffusionModelUNet(**cases.UNET_CASES["unet3d"]["kwargs"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.zeros(1, 1, 8, 8, 8), torch.zeros(1, dtype=torch.long))


def test_arena_layout_keeps_fused_tensors_adjacent():
    from medical_image_generation_amd import engine as E
    from medical_image_generation_amd.unet import DiffusionModelUNet
    net = DiffusionModelUNet(**cases.UNET_CASES["unet3d"]["kwargs"])
    a = E.ParamArena(net._entries, "cpu")
    q = [f"middle_block.attention.to_{t}.weight" for t in "qkv"]
    assert a.span(q).numel() == 3 * 64 * 64
    te = [r[0] + ".time_emb_proj.weight" for r in net._resnets]
    assert a.span(te).numel() == net._temb_total * net.temb_dim
    # statically unused tensors sit behind the trainable prefix
    assert all(a.offsets[n] >= a.n_trainable for n, _, t in net._entries if not t)
    assert all(a.offsets[n] < a.n_trainable for n, _, t in net._entries if t)


def test_discriminator_state_dict_names_match_the_restated_upstream_module():
    """PatchDiscriminator (third-party `generative` class, restated in oracle/disc.py: PARITY UNPINNED): same state_dict names, shapes and
    order -- upstream checkpoints of the discriminator load."""
    from medical_image_generation_amd.discriminator import PatchDiscriminator
    from oracle import disc as odisc
    kw = dict(spatial_dims=3, num_channels=64, in_channels=1, out_channels=1, num_layers_d=3)  # configuration.py:966-967
    net, ref = PatchDiscriminator(**kw), odisc.PatchDiscriminator(**kw)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    net.load_state_dict(ref.state_dict())
