"""16-bit destinations of the all-pairs head (mdg_bilinear_allpairs16_ld): what can be checked without a GPU -- the layout of
``empty_scores(dtype=...)``, the declared entry point, its workspace query and the wrapper's refusals."""
import ctypes

import pytest
import torch

from madrigal_amd import _lib, ops


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("Nt", [1, 63, 64, 65, 300, 1001])
def test_empty_scores_16bit_pitch_is_one_line_of_64_elements(dtype, Nt):
    t = ops.empty_scores(3, 5, Nt, "cpu", dtype=dtype)
    assert t.dtype == dtype and tuple(t.shape) == (3, 5, Nt)
    assert t.stride(2) == 1 and t.stride(1) % 64 == 0 and t.stride(1) >= Nt and t.stride(1) - Nt < 64
    assert t.stride(0) == 5 * t.stride(1)
    assert t.is_contiguous() == (Nt % 64 == 0)


@pytest.mark.parametrize("Nt", [1, 31, 32, 33, 64, 300])
def test_empty_scores_fp32_pitch_is_unchanged(Nt):
    for t in (ops.empty_scores(2, 4, Nt, "cpu"), ops.empty_scores(2, 4, Nt, "cpu", dtype=torch.float32)):
        assert t.dtype == torch.float32 and tuple(t.shape) == (2, 4, Nt)
        assert t.stride(1) == (Nt + 31) // 32 * 32 and t.stride(0) == 4 * t.stride(1)
        assert t.is_contiguous() == (Nt % 32 == 0)


def test_empty_scores_refuses_other_dtypes():
    with pytest.raises(ValueError):
        ops.empty_scores(1, 1, 1, "cpu", dtype=torch.int8)


def test_entry_point_is_declared_with_its_prototype():
    assert "mdg_bilinear_allpairs16_ld" in _lib.declared_symbols()
    restype, argtypes = _lib.declared_prototypes()["mdg_bilinear_allpairs16_ld"]
    p, i64, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert restype is ctypes.c_int
    # z_head, z_tail, w_sym, out, ldo, n_head, n_tail, n_labels, D, precision, epilogue, score_type, workspace, workspace_bytes, stream
    assert argtypes == [p, p, p, p, i64, i64, i64, i64, i64, i, i, i, p, ctypes.c_size_t, p]
    assert hasattr(_lib.lib(), "mdg_bilinear_allpairs16_ld")
    assert _lib.lib().mdg_abi_version() >= 23
    assert ops.SCORE_TYPES == {torch.float16: 1, torch.bfloat16: 2}


def test_workspace_query_is_the_fp32_heads_and_needs_no_gpu():
    L = _lib.lib()
    assert L.mdg_bilinear_allpairs_workspace_bytes(4096, 4096, 896, 128, ops.PREC_F32) == 0
    one = L.mdg_bilinear_allpairs_workspace_bytes(4003, 4003, 901, 128, ops.PREC_F16)
    assert one == L.mdg_bilinear_allpairs_workspace_bytes(4003, 4003, 901, 128, ops.PREC_BF16) > 0
    assert L.mdg_bilinear_allpairs_workspace_bytes(4003, 4003, 901, 128, ops.PREC_BF16X3) == 2 * one


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_16bit_head_refuses_cpu_tensors(dtype):
    z, w = torch.zeros(4, 128), torch.zeros(2, 128, 128)
    with pytest.raises(ValueError, match="GPU"):
        ops.bilinear_allpairs(z, z, w, out_dtype=dtype)
    with pytest.raises(ValueError, match="GPU"):
        ops.bilinear_allpairs(z, z, w, out=torch.zeros(2, 4, 4, dtype=dtype))


def test_unknown_out_dtype_is_refused_before_anything_else():
    z, w = torch.zeros(4, 128), torch.zeros(2, 128, 128)
    for bad in (torch.int8, torch.float64):
        with pytest.raises(ValueError, match="out_dtype"):
            ops.bilinear_allpairs(z, z, w, out_dtype=bad)


@pytest.mark.parametrize("epi", [ops.EPI_ROWSTATS, ops.EPI_TRIKEYS])
def test_16bit_has_no_rowstats_or_keys(epi):
    z, w = torch.zeros(4, 128), torch.zeros(2, 128, 128)
    with pytest.raises(ValueError, match="16-bit"):
        ops.bilinear_allpairs(z, z, w, epilogue=epi, out_dtype=torch.float16)


def test_dtype_and_out_must_agree():
    z, w = torch.zeros(4, 128), torch.zeros(2, 128, 128)
    with pytest.raises(ValueError, match="does not match"):
        ops.bilinear_allpairs(z, z, w, out_dtype=torch.float16, out=torch.zeros(2, 4, 4, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="does not match"):
        ops.bilinear_allpairs(z, z, w, out_dtype=torch.bfloat16, out=torch.zeros(2, 4, 4))
