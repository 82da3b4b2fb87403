"""ctypes binding of libunidistill_hip.so + per-device scratch workspace.

The library is a plain C ABI (no torch types).  torch is imported first so that the HIP runtime
(libamdhip64.so.7) already mapped by torch is the one our library binds to.

The signatures are not written down here: they are parsed from the prototypes of include/unidistill_hip.h at import.
`load()` is the raw CDLL with those argtypes (a call returns its status); `ud` holds the same functions for the product
path: a tensor is accepted wherever the header has a pointer, and a non-zero status raises.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "libunidistill_hip.so")
_cdll = None

c_void_p, c_int = ctypes.c_void_p, ctypes.c_int

HEADER_PATH = os.path.join(_HERE, "..", "..", "include", "unidistill_hip.h")

_SCALARS = {
    "void": None, "int": c_int, "int32_t": c_int, "unsigned": ctypes.c_uint, "uint32_t": ctypes.c_uint,
    "int64_t": ctypes.c_int64, "long long": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
    "double": ctypes.c_double, "ud_stream_t": c_void_p,
}
# Out-parameters that Python passes with byref() of a typed scalar; every other pointer is an address (c_void_p).
_TYPED_POINTERS = {"ud_prof_read": {"double *": ctypes.POINTER(ctypes.c_double), "int *": ctypes.POINTER(c_int)}}
# Entry points whose int result is a value (a count, a flag, ud_jpeg_parse's positive codes), not a UD_ERR_* status.
VALUE_RETURNS = ("ud_abi_version", "ud_voxelize_capacity", "ud_optim_chunk_elems", "ud_conv1x1_f32_persistent_enabled",
                 "ud_conv3x3_wino4_f32_blocks", "ud_conv3x3_wino_f32_blocks", "ud_jpeg_parse",
                 "ud_conv3x3_wino4_f32_block_shape", "ud_head_tail_f32_strip_rows")

_PROTO = re.compile(r"([^;{}()]*?)\b(ud_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")


def _ctype(decl, proto, named):
    """ctypes type of one C declarator (`const float* x`, `long long P`, a bare return type); raises on an unknown spelling."""
    toks = [t for t in re.findall(r"\w+|\*|\S", decl) if t != "const"]
    if "*" in toks:
        spelled = " ".join(toks[:len(toks) - toks[::-1].index("*")])
        typed = _TYPED_POINTERS.get(proto, {}).get(spelled)
        return typed or (ctypes.c_char_p if spelled == "char *" else c_void_p)
    if named and len(toks) > 1 and " ".join(toks) not in _SCALARS:
        toks = toks[:-1]  # the parameter's name
    if " ".join(toks) not in _SCALARS:
        raise ValueError(f"unidistill_hip.h: unknown type {decl.strip()!r} in the prototype of {proto}")
    return _SCALARS[" ".join(toks)]


def parse_header(text):
    """name -> (restype, argtypes) of every ud_* prototype in the header text."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    sigs = {}
    for ret, name, params in _PROTO.findall(text):
        params = [] if params.strip() in ("", "void") else params.split(",")
        sigs[name] = (_ctype(ret, name, False), [_ctype(p, name, True) for p in params])
    stray = set(re.findall(r"\b(ud_[a-z0-9_]+)\s*\(", text)) - set(sigs)
    if stray:
        raise ValueError(f"unidistill_hip.h: cannot parse the prototype of {sorted(stray)[0]}")
    return sigs


with open(HEADER_PATH) as _f:
    _PROTOTYPES = parse_header(_f.read())
assert set(VALUE_RETURNS) <= set(_PROTOTYPES), sorted(set(VALUE_RETURNS) - set(_PROTOTYPES))


class HipLibraryMissing(RuntimeError):
    pass


class _TensorPointer:
    """c_void_p argtype of the checked functions: a tensor goes in as its address (the call's argument tuple keeps it alive
    until the C function returns); None, ints, ctypes arrays and byref() convert as for c_void_p.  The device is not looked
    at (some entry points take host buffers; require_gpu is the callers' check)."""

    @staticmethod
    def from_param(v, _tensor=torch.Tensor, _pointer=c_void_p.from_param):
        # c_void_p.from_param makes a pointer-sized parameter of the address without building a Python-level c_void_p
        # (host cost per argument: the wrappers are launch-bound); a bare int returned from here would go in as a 32-bit C int
        return _pointer(v.data_ptr() if isinstance(v, _tensor) else v)


def _raise_on_error(code, fn, args):
    if code:
        check(code, fn.__name__)
    return code


class _CheckedLibrary:
    """`_lib.ud`: every entry point once more, taking tensors for pointers and raising on a non-zero status."""

    def __getattr__(self, name):  # only reached while load() has not filled the instance yet
        if _cdll is None:
            load()
            return getattr(self, name)
        raise AttributeError(name)


ud = _CheckedLibrary()


def load():
    """Return the loaded CDLL; raise HipLibraryMissing (never fall back) if it is not built."""
    global _cdll
    if _cdll is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryMissing(
                f"{LIB_PATH} not found: build it with `make -C cvpr2023-unidistill_amd` "
                "(or __graft_entry__.build()). There is no CPU fallback.")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOTYPES.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = res, args
            checked = lib[name]  # a second function object: the raw one keeps returning its status
            checked.restype = res
            checked.argtypes = [_TensorPointer if a is c_void_p else a for a in args]
            if res is c_int and name not in VALUE_RETURNS:
                checked.errcheck = _raise_on_error
            setattr(ud, name, checked)
        _cdll = lib
    return _cdll


def exported_symbols():
    return sorted(_PROTOTYPES)


def check(code, what):
    if code != 0:
        msg = load().ud_error_string(code).decode()
        raise RuntimeError(f"{what} failed: {msg} ({code})")


def ptr(t):
    """Device address as a plain int (ctypes converts it for a c_void_p parameter; None -> NULL)."""
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_of(t):
    """hipStream_t torch is currently enqueuing on for t's device (host cost matters: the wrappers are
    launch-bound at small batches, so this avoids building a torch.cuda.Stream object per call)."""
    if _raw_stream is not None:
        idx = t.device.index
        return _raw_stream(idx if idx is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(t.device).cuda_stream


# Strict mode: a branch of the product path that would leave the hand-written kernels for a library convolution / GEMM
# (nn.Conv2d -> MIOpen, `@` -> hipBLASLt, aten.convolution_backward) raises instead, naming the site and the shape.
# UD_STRICT=1 (bench.py and the test-suite default); `strict(False)` scopes the lenient behaviour (goldens at shrunk widths).
STRICT = os.environ.get("UD_STRICT", "0") == "1"


class strict:
    def __init__(self, on):
        self.on = bool(on)

    def __enter__(self):
        global STRICT
        self.prev, STRICT = STRICT, self.on
        return self

    def __exit__(self, *exc):
        global STRICT
        STRICT = self.prev
        return False


def library_fallthrough(site, *tensors, **info):
    """Called right before a GPU tensor is handed to a library convolution / GEMM from a module that has a hand-written path."""
    if not STRICT or not any(t is not None and t.is_cuda for t in tensors):
        return
    shapes = ", ".join(f"{tuple(t.shape)} {str(t.dtype).replace('torch.', '')} strides {tuple(t.stride())}"
                       for t in tensors if t is not None)
    extra = "".join(f", {k}={v}" for k, v in info.items())
    raise RuntimeError(f"UD_STRICT: {site} would fall through to a library kernel for {shapes}{extra} "
                       "(no hand-written kernel accepts this shape / layout; set UD_STRICT=0 to allow the library path)")


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("unidistill_amd ops run on the GPU only (no CPU fallback); "
                               f"got a tensor on {t.device}")


def require_gpu_device(device):
    """torch.device(device), which must be a GPU."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("unidistill_amd ops run on the GPU only (no CPU fallback); got device " + str(device))
    return device


_workspaces = {}
_scope = ["eager"]


class workspace_scope:
    """Workspaces requested inside the scope get their own buffers.  A captured hipGraph bakes the
    scratch pointers in, so a graph must never share (or lose to a re-allocation) the buffers that
    eager code may grow later."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        _scope.append(self.name)

    def __exit__(self, *a):
        _scope.pop()


def workspace(device, nbytes, slot="default"):
    """Grow-only byte scratch per (device, scope, slot); stream-ordered reuse on torch's stream."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), _scope[-1], slot)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"workspace {key} would be re-allocated during graph capture")
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = buf
    return buf


def prof_enable(on=True):
    load().ud_prof_enable(1 if on else 0)


def prof_read(name, reset=True):
    """-> (total_ms, calls) of the named kernel since the last reset (blocks on its events)."""
    ms, n = ctypes.c_double(0.0), c_int(0)
    check(load().ud_prof_read(name.encode(), ctypes.byref(ms), ctypes.byref(n), 1 if reset else 0),
          "ud_prof_read")
    return ms.value, n.value
