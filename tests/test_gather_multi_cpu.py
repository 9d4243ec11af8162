"""CPU checks of the multi-source row gather: mdg_gather_rows_multi is declared, typed and exported, the C entry refuses bad
arguments before it touches a device, and the wrapper validates (the HIP path has no CPU fallback)."""
import ctypes

import pytest
import torch


def test_symbol_is_declared_typed_and_exported():
    from madrigal_amd import _lib
    L = _lib.lib()
    s = "mdg_gather_rows_multi"
    assert s in _lib.declared_symbols() and hasattr(L, s)
    P, I, I64, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    assert _lib.declared_prototypes()[s] == (I, [P, P, P, I, I64, I64, P, I64, P, I64, P, Z, I, P])
    assert L.mdg_abi_version() >= 17


def test_c_entry_refuses_before_it_touches_a_device():
    from madrigal_amd._lib import lib
    L = lib()
    f = L.mdg_gather_rows_multi
    ptrs = (ctypes.c_void_p * 2)(4096, 8192)
    rows = (ctypes.c_int64 * 2)(5, 5)
    ld = (ctypes.c_int64 * 2)(128, 128)
    out = 1 << 20
    for args, what in (((ptrs, rows, ld, 0, 5, 128, 64, 3, out, 128, None, 0, 1, None), b"sources"),
                       ((ptrs, rows, ld, 20, 5, 128, 64, 3, out, 128, None, 0, 1, None), b"sources"),
                       ((None, rows, ld, 2, 5, 128, 64, 3, out, 128, None, 0, 1, None), b"null source table"),
                       ((ptrs, rows, ld, 2, 0, 128, 64, 3, out, 128, None, 0, 1, None), b"bad size"),
                       ((ptrs, rows, ld, 2, 5, 128, 64, 3, None, 0, None, 0, 1, None), b"neither"),
                       ((ptrs, rows, ld, 2, 5, 128, None, 3, out, 128, None, 0, 1, None), b"null index"),
                       ((ptrs, rows, ld, 2, 4, 128, 64, 3, out, 128, None, 0, 1, None), b"rows_per_source"),        # a source longer than the divisor
                       ((ptrs, rows, ld, 2, 5, 132, 64, 3, out, 132, None, 0, 1, None), b"width"),                 # ld < width
                       ((ptrs, rows, ld, 2, 5, 128, 64, 3, out, 126, None, 0, 1, None), b"ldo"),
                       ((ptrs, rows, ld, 2, 5, 128, 64, 3, out + 4, 128, None, 0, 1, None), b"16-byte"),
                       ((ptrs, rows, ld, 2, 5, 128, 64, 3, None, 0, out, 1 << 20, 0, None), b"16-bit")):
        assert f(*args) == -1 and b"mdg_gather_rows_multi" in L.mdg_last_error() and what in L.mdg_last_error(), (what, L.mdg_last_error())
    assert f(ptrs, rows, ld, 2, 5, 128, 64, 3, None, 0, out, 16, 1, None) == -2 and b"image of" in L.mdg_last_error()
    assert f(ptrs, rows, ld, 2, 5, 128, None, 0, out, 128, None, 0, 1, None) == 0                # no row: nothing to do


def test_wrapper_validation_without_a_gpu():
    from madrigal_amd import ops
    a, idx = torch.zeros(4, 128), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="1 to 19 sources"):
        ops.gather_rows_multi([], idx)
    with pytest.raises(ValueError, match="1 to 19 sources"):
        ops.gather_rows_multi([a] * 20, idx)
    with pytest.raises(ValueError, match="fp32 cuda matrix"):      # a well-formed call on CPU tensors: no CPU fallback
        ops.gather_rows_multi([a, a], idx)
