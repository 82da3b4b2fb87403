"""CPU: the C-ABI library loads and exports every symbol include/unidistill_hip.h declares; the ctypes signatures are parsed
from that header (unidistill_amd/_lib.py), strictly, and the checked handle `_lib.ud` converts pointers and raises on a status."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _declared():
    """The header's ud_* names by a raw-text regex: the count the parser in _lib.py is held against."""
    text = open(os.path.join(ROOT, "include", "unidistill_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ud_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported(hip_lib):
    names = _declared()
    assert len(names) >= 7
    for n in names:
        assert hasattr(hip_lib, n), f"{n} declared in unidistill_hip.h but not exported"


def test_binding_covers_header(hip_lib):
    from unidistill_amd import _lib
    assert set(_declared()) == set(_lib.exported_symbols())


def test_parser_finds_every_prototype(hip_lib):
    from unidistill_amd import _lib
    parsed = _lib.parse_header(open(os.path.join(ROOT, "include", "unidistill_hip.h")).read())
    assert len(parsed) == len(_declared()) and sorted(parsed) == _declared() == _lib.exported_symbols()
    for name, (res, args) in parsed.items():
        fn = getattr(hip_lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert parsed["ud_prof_read"] == (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_double),
                                                     ctypes.POINTER(ctypes.c_int), ctypes.c_int])
    assert parsed["ud_head_tail_stats"][1][16] is ctypes.c_void_p          # long long* batches_tracked
    assert set(_lib.VALUE_RETURNS) <= set(parsed)


def test_parser_is_strict():
    from unidistill_amd import _lib
    P, I, L, F, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double
    text = """
        /* ud_in_block_comment(int x); */
        // int ud_in_line_comment(int x);
        #define UD_SOMETHING(x) ud_in_macro(x)
        typedef void* ud_stream_t;
        typedef struct UdRec { int64_t a, b; } UdRec;
        int ud_multi(const float* x, int64_t n,
                     const float* const* tables,   /* ud_in_argument_comment( */
                     unsigned flags, const UdRec* recs,
                     long long P, void* workspace, size_t workspace_bytes,
                     ud_stream_t stream);
        size_t ud_bytes(void);
        const char* ud_text(int32_t code, uint32_t u, float f, double d, unsigned char* bytes);
        void ud_switch(int on);
    """
    assert _lib.parse_header(text) == {
        "ud_multi": (I, [P, L, P, ctypes.c_uint, P, L, P, ctypes.c_size_t, P]),
        "ud_bytes": (ctypes.c_size_t, []),
        "ud_text": (ctypes.c_char_p, [I, ctypes.c_uint, F, D, P]),
        "ud_switch": (None, [I]),
    }
    for bad in ("int ud_foo(wchar_t x);", "ud_foo(wchar_t x);", "int ud_foo(int a, short b);", "long ud_foo(int a);",
                "int ud_foo(int (*callback)(int));"):
        with pytest.raises(ValueError, match="ud_foo"):
            _lib.parse_header("int ud_fine(int a);\n" + bad)


def test_checked_call_raises_and_matches_the_raw_call(hip_lib):
    """`_lib.ud` on the host-side entry ud_stem_pack_weights (test_stem_cpu.py): the status becomes an exception that names the
    function and the code; a good call returns 0 and writes the bytes the raw call writes."""
    from unidistill_amd import _lib
    w = np.random.default_rng(7).standard_normal((64, 3, 7, 7)).astype(np.float32)
    sn, sc, sky, skx = (s // 4 for s in w.strides)
    raw, chk = (np.full(7 * 6 * 4 * 16 * 4, np.nan, np.float32) for _ in range(2))
    assert hip_lib.ud_stem_pack_weights(w.ctypes.data, sn, sc, sky, skx, raw.ctypes.data) == 0
    assert _lib.ud.ud_stem_pack_weights(w.ctypes.data, sn, sc, sky, skx, chk.ctypes.data) == 0
    assert not np.isnan(raw).any() and raw.tobytes() == chk.tobytes()
    code = hip_lib.ud_stem_pack_weights(None, sn, sc, sky, skx, raw.ctypes.data)       # the raw handle still returns the status
    assert code != 0
    with pytest.raises(RuntimeError, match=rf"ud_stem_pack_weights failed: .* \({code}\)"):
        _lib.ud.ud_stem_pack_weights(None, sn, sc, sky, skx, chk.ctypes.data)
    assert _lib.ud.ud_stem_pack_weights is not hip_lib.ud_stem_pack_weights
    assert getattr(hip_lib.ud_stem_pack_weights, "errcheck", None) is None
    for name in _lib.VALUE_RETURNS:                                                     # values, not statuses: never checked
        assert getattr(getattr(_lib.ud, name), "errcheck", None) is None, name
    assert _lib.ud.ud_abi_version() == hip_lib.ud_abi_version() >= 1


def test_pointer_conversion(hip_lib):
    """What the checked functions accept for a pointer: a tensor (its data_ptr(), as a c_void_p), None, an int with all 64
    bits, a ctypes array, byref(); then one real call with tensors."""
    import torch
    from unidistill_amd import _lib
    conv = _lib.ud.ud_stem_pack_weights.argtypes[0].from_param
    t = torch.arange(6, dtype=torch.float32)[2:]                          # data_ptr() is not the storage's first byte
    address = lambda param: ctypes.cast(param, ctypes.c_void_p).value
    assert not isinstance(conv(t), int) and address(conv(t)) == t.data_ptr()     # a bare int would be passed as a 32-bit C int
    assert address(conv(torch.nn.Parameter(t))) == t.data_ptr()
    assert conv(None) is None
    big = conv(ctypes.c_void_p(1 << 40).value + 4)                         # the int branch keeps all 64 bits
    assert address(big) == (1 << 40) + 4
    arr, one = (ctypes.c_int * 9)(*range(9)), ctypes.c_int(5)
    assert address(conv(arr)) == ctypes.addressof(arr)
    assert conv(ctypes.byref(one)) is not None
    with pytest.raises((TypeError, ctypes.ArgumentError)):
        conv(1.5)
    # end to end, tensors for both pointers: with unit strides the packer reads w[n + c + ky + kx], at most element 77
    src = torch.full((80,), 3.25)
    out = torch.zeros(7 * 6 * 4 * 16 * 4)
    assert _lib.ud.ud_stem_pack_weights(src, 1, 1, 1, 1, out) == 0 and float(out[0]) == 3.25


def test_identity(hip_lib):
    assert hip_lib.ud_version().decode().startswith("unidistill_hip")
    assert hip_lib.ud_abi_version() >= 1
    assert hip_lib.ud_error_string(-2).decode().startswith("workspace")


def test_workspace_queries_are_pure(hip_lib):
    n = hip_lib.ud_bev_pool_workspace_bytes(1, 473088, 256, 180, 180, 1)
    assert n > 3 * 473088 * 4
    assert hip_lib.ud_bev_pool_workspace_bytes(0, 1, 1, 1, 1, 1) == 0


def test_no_cpu_fallback():
    """Product ops must refuse CPU tensors instead of silently computing elsewhere."""
    import pytest
    import torch
    from unidistill_amd.ops import bev_pool
    geom = torch.zeros(1, 4, 3, dtype=torch.int32)
    feat = torch.zeros(1, 4, 4)
    with pytest.raises(RuntimeError, match="GPU only"):
        bev_pool.voxel_pooling(geom, feat, (2, 2, 1))
