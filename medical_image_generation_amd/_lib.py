"""ctypes binding of libmedimgen_hip.so (the C ABI declared in include/medimgen_hip.h).

There is NO fallback: if the library is missing or a call fails, a RuntimeError is raised.
PyTorch is used only as the owner of device memory and streams; every pointer handed to the
library is `tensor.data_ptr()`.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MI_LIB_PATH") or os.path.join(_HERE, "libmedimgen_hip.so")  # MI_LIB_PATH: ablation builds (csrc/Makefile `diag`)

HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "medimgen_hip.h")  # the library is only built and used in-tree

_C_TYPES = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "hipStream_t": C.c_void_p}
_C_RETURNS = ("int", "int64_t")
_ENUM = re.compile(r"\benum\b\s*\w*\s*\{([^}]*)\}\s*;")


def _parse_header(text: str):
    """The C ABI from the header's text (no I/O): ({entry point: (restype, [argtypes])}, {MI_* macro or enumerator: int}).
    Arguments map by ABI class -- every pointer (`*`, `T name[3]`, hipStream_t) is c_void_p -- and a declaration this does not
    understand is an error, never an `int` by default: a wrong class resolves the symbol and then reads shifted arguments."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)  # first: the comments hold parentheses, commas and mi_*( call-like text
    constants = {m[1]: int(m[2]) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(MI_\w+)[ \t]+(-?\d+)[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    for body in _ENUM.findall(text):
        for item in filter(str.strip, body.split(",")):
            m = re.fullmatch(r"\s*(\w+)\s*=\s*(-?\d+)\s*", item)
            if not m:
                raise RuntimeError(f"medimgen_hip.h: enumerator `{item.strip()}` has no explicit integer value")
            constants[m[1]] = int(m[2])
    functions = {}
    for decl in re.sub(r'extern\s*"C"\s*\{|\}', " ", _ENUM.sub(" ", text)).split(";"):
        if "(" not in decl:  # typedefs of the opaque handles
            continue
        decl = " ".join(decl.split())

        def argtype(param):
            words = [w for w in param.split() if w != "const"]
            if "*" in param or param.rstrip().endswith("]"):
                return C.c_void_p
            if not 1 <= len(words) <= 2 or words[0] not in _C_TYPES:
                raise RuntimeError(f"medimgen_hip.h: parameter `{param.strip()}` of `{decl};` is of no supported ABI class")
            return _C_TYPES[words[0]]

        m = re.fullmatch(r"(.*?)\s*\b(mi_\w+)\s*\(([^()]*)\)", decl)
        if not m or m[1] not in _C_RETURNS or m[2] in functions:
            raise RuntimeError(f"medimgen_hip.h: `{decl};` is no `int|int64_t mi_name(params);` declaration (or a second one of its name)")
        params = [] if m[3].strip() in ("", "void") else m[3].split(",")
        functions[m[2]] = (_C_TYPES[m[1]], [argtype(p) for p in params])
    return functions, constants


@functools.cache
def _header():
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError(f"{HEADER_PATH} is missing: the binding of libmedimgen_hip.so is derived from it")
    with open(HEADER_PATH) as f:
        return _parse_header(f.read())


def constants() -> dict[str, int]:
    """The integer `#define MI_*` macros and the enumerators of the header.  Needs no library (CPU-only hosts read them too)."""
    return _header()[1]


def exported_symbols() -> list[str]:
    return sorted(_header()[0])


def signature(name: str):
    """(restype, argtypes) of an entry point as load() sets them."""
    return _header()[0][name]


# The entry points that return a value instead of a status (call_raw does not check them).
_NOCHECK = {"mi_abi_version", "mi_pp_stats_workspace_bytes", "mi_meter_bytes", "mi_ssim_tiles", "mi_gn_small_supported", "mi_conv1x1_skip_fusable", "mi_gn_workspace_bytes", "mi_aug_stats_workspace_bytes", "mi_attn_supported", "mi_attn_workspace_bytes", "mi_conv_fwd_stats_chunks",
            "mi_conv2d_k4_wgrad_splits", "mi_conv2d_k4_edge_wgrad_splits", "mi_conv_last_kernel", "mi_conv_plan_wgrad_splits",
            "mi_dm_gram_workspace_bytes", "mi_dm_gram_single_pass", "mi_dm_jacobi_max_sweeps", "mi_dm_jacobi_single_workgroup"}

_lib = None
# Version of the C ABI (MI_ABI_VERSION of the header, which csrc/api.hip returns).  Entry points have changed their argument lists under
# unchanged names between versions, and *.so files are not tracked by git: a stale library (or an MI_LIB_PATH pointing at an old
# ablation build) resolves every symbol and then reads shifted arguments.  load() refuses it.
ABI_VERSION = constants()["MI_ABI_VERSION"]


def load():
    """dlopen the library (once) and bind every entry point the header declares.  Raises RuntimeError when it has not been built."""
    global _lib
    if _lib is None:
        functions = _header()[0]
        if _NOCHECK - set(functions):
            raise RuntimeError(f"_lib._NOCHECK names entry points that {HEADER_PATH} does not declare: {sorted(_NOCHECK - set(functions))}")
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU / PyTorch fallback for the HIP path)")
        lib = C.CDLL(LIB_PATH)
        try:
            lib.mi_abi_version.restype = C.c_int
            have = int(lib.mi_abi_version())
        except AttributeError:
            have = None
        if have != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} is a stale library (C ABI {have}, this binding needs {ABI_VERSION}): rebuild it with "
                               "`python -c 'import __graft_entry__ as g; g.build()'`")
        for name, (restype, argtypes) in functions.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:  # entry points added without a version change (mi_sw_*, then mi_sw_*_cl / mi_sw_diffusion_step, then mi_dm_*): a library built before them is stale too
                raise RuntimeError(f"{LIB_PATH} is a stale library (it lacks {name}): rebuild it with "
                                   "`python -c 'import __graft_entry__ as g; g.build()'`") from None
            fn.argtypes, fn.restype = argtypes, restype
        _lib = lib
    return _lib


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


class HipError(RuntimeError):
    pass


_ERRS = {constants()["MI_ERR_BAD_ARG"]: "MI_ERR_BAD_ARG (host-side shape/alignment check failed)", constants()["MI_ERR_UNSUPPORTED"]: "MI_ERR_UNSUPPORTED"}


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_cuda, "medimgen HIP ops take device tensors only"
    return t.data_ptr()


_profile = None


class profile_calls:
    """Context manager: HIP events on the launch stream around every library call made inside it (eager mode only -- events cannot
    be recorded into a capturing stream this way); summary() -> {entry point: GPU milliseconds}.  Measurement aid for bench.py."""

    def __enter__(self):
        global _profile
        self.records = []
        _profile = self
        return self

    def __exit__(self, *exc):
        global _profile
        _profile = None
        return False

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1 in self.records:
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
        return out


def call(name: str, *args):
    """Invoke `name` on the current stream (appended as the last argument) and check the status."""
    fn = getattr(load(), name)
    prof = _profile
    if prof is not None:
        st = torch.cuda.current_stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
    rc = fn(*args, stream_ptr())
    if prof is not None:
        e1.record(st)
        prof.records.append((name, e0, e1))
    if rc != 0:
        raise HipError(f"{name} failed: {_ERRS.get(rc, f'hipError_t {rc}')}")


def call_raw(name: str, *args):
    fn = getattr(load(), name)
    rc = fn(*args)
    if name not in _NOCHECK and rc != 0:
        raise HipError(f"{name} failed: {_ERRS.get(rc, f'hipError_t {rc}')}")
    return rc
