"""CPU checks of the drop-in boundary: the C-ABI library loads and exports every declared symbol."""
import ctypes
import os

import pytest


def test_library_exports_every_declared_symbol():
    from madrigal_amd import _lib
    syms = _lib.declared_symbols()
    assert "mdg_bilinear_allpairs" in syms and "mdg_last_error" in syms
    L = _lib.lib()
    for s in syms:
        assert hasattr(L, s), s
    assert L.mdg_build_arch() == b"gfx950"
    assert L.mdg_abi_version() >= 1


def test_workspace_queries_need_no_gpu():
    from madrigal_amd import _lib
    L = _lib.lib()
    c = ctypes.c_int64
    assert L.mdg_bilinear_allpairs_workspace_bytes(c(4096), c(4096), c(896), c(128), 0) == 0
    b3 = L.mdg_bilinear_allpairs_workspace_bytes(c(4096), c(4096), c(896), c(128), 1)
    b1 = L.mdg_bilinear_allpairs_workspace_bytes(c(4096), c(4096), c(896), c(128), 2)
    assert b3 == 2 * b1 and b1 >= 4096 * 128 * 2 + 896 * 128 * 128 * 2


def test_dense_block_tile_query_needs_no_gpu(monkeypatch):
    """mdg_linear_tile / ops.linear_tile: the launch path's own choice between the 256- and the 128-tile kernel -- 16-bit mode,
    M >= 1024, N >= 256 and at least 192 tiles of 256 x 256 -- and the MDG_LINEAR_TILE switch, re-read after a reload."""
    from helpers import set_switch
    from madrigal_amd import _lib, ops
    monkeypatch.delenv("MDG_LINEAR_TILE", raising=False)
    _lib.lib().mdg_tuning_reload()
    for M, N in ((1023, 49152), (4097, 2048), (1024, 12288), (3100, 3800), (1, 1), (22016, 6144)):
        assert ops.linear_tile(M, N, "f32") == 128, (M, N)
    for prec in ("bf16", "bf16x3"):
        assert ops.linear_tile(1023, 49152, prec) == 128                  # 4 x 192 tiles, but M < 1024
        assert ops.linear_tile(4097, 2048, prec) == 128                   # 17 x 8 = 136 tiles
        assert ops.linear_tile(1024, 12288, prec) == 256                  # 4 x 48 = 192 tiles
        assert ops.linear_tile(3100, 3800, prec) == 256                   # 13 x 15 = 195 tiles
        assert ops.linear_tile(22016, 6144, prec) == 256
    assert _lib.lib().mdg_linear_tile(3100, 3800, ops.PREC_BF16) == 256
    set_switch(monkeypatch, "MDG_LINEAR_TILE", "256")
    assert ops.linear_tile(1, 1, "bf16") == 256 and ops.linear_tile(1, 1, "bf16x3") == 256 and ops.linear_tile(1, 1, "f32") == 128
    set_switch(monkeypatch, "MDG_LINEAR_TILE", "128")
    for prec in ("f32", "bf16", "bf16x3"):
        assert ops.linear_tile(22016, 6144, prec) == 128
    monkeypatch.delenv("MDG_LINEAR_TILE")
    _lib.lib().mdg_tuning_reload()
    assert ops.linear_tile(22016, 6144, "bf16") == 256 and ops.linear_tile(1, 1, "bf16") == 128


def test_ops_refuse_cpu_tensors():
    import torch
    from madrigal_amd import ops
    z = torch.zeros(4, 128)
    w = torch.zeros(1, 128, 128)
    with pytest.raises(ValueError, match="GPU"):
        ops.bilinear_allpairs(z, z, w)


def test_missing_library_is_loud(monkeypatch, tmp_path):
    from madrigal_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", os.path.join(tmp_path, "nope.so"))
    with pytest.raises(_lib.MadrigalHipError):
        _lib.lib()


def test_prototypes_cover_every_declared_symbol():
    from madrigal_amd import _lib
    protos = _lib.declared_prototypes()
    assert sorted(protos) == _lib.declared_symbols()
    L = _lib.lib()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is restype, name
        assert list(fn.argtypes) == argtypes, name
    assert protos["mdg_last_error"] == (ctypes.c_char_p, []) and protos["mdg_tuning_reload"] == (None, [])
    assert protos["mdg_symmetrize"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p])
    assert protos["mdg_gmean"][1][0] is ctypes.c_void_p                       # const float* const*
    assert protos["mdg_pack_operand_bytes"] == (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int])


@pytest.mark.parametrize("proto", ["int mdg_x(int64_t n, long flags, void* stream);", "unsigned mdg_x(int64_t n);",
                                   "int mdg_x(unsigned int n);", "struct mdg_s mdg_x(void);", "float* mdg_x(void);"])
def test_unknown_type_spelling_raises(proto):
    from madrigal_amd import _lib
    with pytest.raises(_lib.MadrigalHipError, match="mdg_x"):
        _lib.parse_prototypes(proto)


def test_size_queries_are_full_width():
    """Host-only size queries with bare Python ints: results above 2^32 and one argument above 2^31 arrive whole."""
    from madrigal_amd import _lib, ops
    L = _lib.lib()
    image = 8_000_000 * 256 * 4
    assert image > 2 ** 32
    assert L.mdg_pack_operand_bytes(8_000_000, 256, ops.PREC_BF16X3) >= image
    assert L.mdg_linear_backward_pack_bytes(8_000_000, 256, ops.PREC_BF16X3, 0) >= image
    assert L.mdg_label_metrics_workspace_bytes(3_000_000_000, 896) >= 16 * 3_000_000_000


def test_typed_calls_reject_wrong_arguments():
    from madrigal_amd import _lib
    L = _lib.lib()
    with pytest.raises(TypeError):
        L.mdg_pack_operand_bytes(1024, 256)                                   # one argument too few
    with pytest.raises(ctypes.ArgumentError):
        L.mdg_pack_operand_bytes(1024.0, 256, 1)                              # a float for an int64_t
    with pytest.raises(ctypes.ArgumentError):
        L.mdg_symmetrize(3.5, None, 1, 128, None)                             # a float for a pointer


def test_checked_call_honours_a_patched_symbol(monkeypatch):
    from madrigal_amd import _lib
    L = _lib.lib()
    seen = []

    def refusing(*args):
        seen.append(args)
        return -1
    monkeypatch.setattr(L, "mdg_symmetrize", refusing)
    with pytest.raises(ValueError, match="^mdg_symmetrize: "):
        _lib.call("mdg_symmetrize", None, None, 1, 128, None)
    with pytest.raises(ValueError, match="^some label: "):
        _lib.call("mdg_symmetrize", None, None, 1, 128, None, what="some label")
    assert seen == [(None, None, 1, 128, None)] * 2
    monkeypatch.setattr(L, "mdg_symmetrize", lambda *args: -3)
    with pytest.raises(_lib.MadrigalHipError, match=r"mdg_symmetrize failed \(code -3\)"):
        _lib.call("mdg_symmetrize", None, None, 1, 128, None)
    assert _lib.call("mdg_lars_multi", None, None, None, None, None, None, 0, 0, None, 0, None) is None    # status 0: no device touched


def test_no_hand_marshalling_outside_the_binding():
    import re
    from madrigal_amd import _lib
    spelling = re.compile(r"_c64\(|_vp\(|ctypes\.c_size_t\(|ctypes\.c_int64\(|ctypes\.c_void_p\(")
    for f in sorted(os.listdir(_lib.HERE)):
        if f.endswith(".py") and f != "_lib.py":
            hits = [ln for ln in open(os.path.join(_lib.HERE, f)) if spelling.search(ln)]
            assert not hits, (f, hits)
