"""CPU checks of the threshold selection of the all-pairs head: the C ABI of mdg_bilinear_select_* is declared, typed and exported,
its workspace is the operand images, the wrappers validate before they touch a device, pipeline.csr_rows expands row pointers
exactly, and the dense-to-CSR reference of the GPU tests is right on a hand-checked tensor."""
import ctypes

import pytest
import torch

from select_ref import csr_of_mask, dense_csr, dense_mask

NEW = ("mdg_bilinear_select_workspace_bytes", "mdg_bilinear_select_count", "mdg_bilinear_select_fill")


def test_select_symbols_are_declared_typed_and_exported():
    from madrigal_amd import _lib
    syms = _lib.declared_symbols()
    protos = _lib.declared_prototypes()
    L = _lib.lib()
    for s in NEW:
        assert s in syms and s in protos and hasattr(L, s), s
    P, I, I64, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    expected = {
        "mdg_bilinear_select_workspace_bytes": (Z, [I64, I64, I64, I64, I]),
        "mdg_bilinear_select_count": (I, [P, P, P, P, P, I64, I64, I64, I64, I, I, P, Z, P]),
        "mdg_bilinear_select_fill": (I, [P, P, P, P, P, P, P, I64, I64, I64, I64, I, I, P, Z, P]),
    }
    for s, (res, args) in expected.items():
        assert protos[s] == (res, args), (s, protos[s])
        assert getattr(L, s).restype == res and list(getattr(L, s).argtypes) == args, s
    assert L.mdg_abi_version() >= 15


def test_select_workspace_is_the_operand_images():
    from madrigal_amd import _lib
    L = _lib.lib()
    assert L.mdg_bilinear_select_workspace_bytes(4096, 4096, 896, 128, 0) == 0
    for nh, nt, nl in ((4096, 4096, 896), (100352, 100352, 64), (7, 333, 3)):
        for prec in (0, 1, 2, 3):
            assert (L.mdg_bilinear_select_workspace_bytes(nh, nt, nl, 128, prec)
                    == L.mdg_bilinear_topk_workspace_bytes(nh, nt, nl, 128, prec, 16))


def test_c_entry_points_refuse_before_they_touch_a_device():
    from madrigal_amd._lib import lib
    L = lib()
    for fn, extra in (("mdg_bilinear_select_count", (None,)), ("mdg_bilinear_select_fill", (None, None, None))):
        f = getattr(L, fn)
        for n_head, n_tail, n_labels, D, eligible, what in ((4, 4, 1, 128, 7, b"unknown eligible"), (4, 5, 1, 128, 2, b"one drug set"),
                                                            (4, 5, 1, 128, 1, b"one drug set"), (4, 4, 1, 64, 0, b"D must be"),
                                                            (4, 4, 65536, 128, 0, b"n_labels"), (4, 0, 1, 128, 0, b"n_tail must be"),
                                                            (4, 4, 1, 128, 0, b"null pointer")):
            rc = f(None, None, None, None, *extra, n_head, n_tail, n_labels, D, 0, eligible, None, 0, None)
            assert rc == -1 and fn.encode() in L.mdg_last_error() and what in L.mdg_last_error(), (fn, what, L.mdg_last_error())
        assert f(None, None, None, None, *extra, 0, 0, 1, 128, 0, 0, None, 0, None) == 0            # no row: nothing to do


def test_wrapper_validation_without_a_gpu():
    from madrigal_amd import ops
    z, z2, w = torch.zeros(6, 128), torch.zeros(4, 128), torch.zeros(2, 128, 128)
    thr = torch.zeros(2)
    for f in (ops.bilinear_select_count, ops.bilinear_select):
        with pytest.raises(ValueError, match="NaN"):
            f(z, z, w, torch.tensor([0.0, float("nan")]))
        with pytest.raises(ValueError, match="one cut per outcome"):
            f(z, z, w, torch.zeros(3))
        with pytest.raises(ValueError, match="1 dims"):
            f(z, z, w, torch.zeros(2, 1))
        with pytest.raises(ValueError, match="float32"):
            f(z, z, w, thr.double())
        with pytest.raises(ValueError, match="one drug set"):
            f(z, z2, w, thr, eligible="lower")
        with pytest.raises(ValueError, match="unknown eligible"):
            f(z, z, w, thr, eligible="upper")
        with pytest.raises(ValueError, match="unknown precision"):
            f(z, z, w, thr, precision="fp8")
        with pytest.raises(ValueError, match="feature dims"):
            f(z[:, :64], z, w, thr)
        # a well-formed call on CPU tensors: the HIP path has no CPU fallback
        with pytest.raises(ValueError, match="GPU"):
            f(z, z, w, thr)
        with pytest.raises(ValueError, match="GPU"):
            f(z, z2, w, torch.tensor([float("-inf"), float("inf")]))
        with pytest.raises(RuntimeError, match="forward-only"):
            f(z.clone().requires_grad_(), z, w, thr)


def test_csr_rows_against_a_hand_built_csr():
    from madrigal_amd.pipeline import csr_rows
    # 3 outcomes x 4 heads; outcome 1 is empty, rows 0, 3 (outcome 0) and 8, 10 (outcome 2) are empty
    counts = [0, 2, 1, 0, 0, 0, 0, 0, 0, 3, 0, 1]
    row_ptr = torch.tensor([0, 0, 2, 3, 3, 3, 3, 3, 3, 3, 6, 6, 7])
    assert row_ptr.diff().tolist() == counts
    l, h, off = csr_rows(row_ptr, 4)
    assert l.tolist() == [0, 0, 0, 2, 2, 2, 2] and h.tolist() == [1, 1, 2, 1, 1, 1, 3] and off.tolist() == [0, 3, 3, 7]
    assert l.dtype == torch.int64 and h.dtype == torch.int64 and off.dtype == torch.int64
    l2, h2, off2 = csr_rows(row_ptr, 4, total=7)
    assert torch.equal(l2, l) and torch.equal(h2, h) and torch.equal(off2, off)
    off[0] = 9
    assert int(row_ptr[0]) == 0                                               # offsets are a copy
    l, h, off = csr_rows(torch.zeros(13, dtype=torch.int64), 4)               # nothing selected at all
    assert l.numel() == 0 and h.numel() == 0 and off.tolist() == [0, 0, 0, 0]
    l, h, off = csr_rows(torch.tensor([0, 5]), 1)                             # one outcome, one head
    assert l.tolist() == [0] * 5 and h.tolist() == [0] * 5 and off.tolist() == [0, 5]
    l, h, off = csr_rows(torch.tensor([0]), 4)                                # no outcome
    assert l.numel() == 0 and off.tolist() == [0]
    for bad, n in ((torch.zeros(12, dtype=torch.int64), 4), (torch.zeros((2, 5), dtype=torch.int64), 4), (torch.zeros(3, dtype=torch.int64), 0)):
        with pytest.raises(ValueError):
            csr_rows(bad, n)


def test_dense_to_csr_reference_on_a_hand_checked_tensor():
    """2 outcomes, 3 x 3; cut 2.0 for outcome 0 (entries equal to 2.0 are selected: >=), +inf for outcome 1; a NaN entry is never
    selected."""
    nan, inf = float("nan"), float("inf")
    dense = torch.tensor([[[2.0, 1.0, 3.0], [0.0, 2.0, 2.0], [5.0, nan, 1.5]],
                          [[9.0, 9.0, 9.0], [9.0, 9.0, 9.0], [9.0, 9.0, 9.0]]])
    thr = torch.tensor([2.0, inf])
    rc, rp, cols, vals = dense_csr(dense, thr, "all")
    assert rc.tolist() == [[2, 2, 1], [0, 0, 0]] and rc.dtype == torch.int32
    assert rp.tolist() == [0, 2, 4, 5, 5, 5, 5] and rp.dtype == torch.int64
    assert cols.tolist() == [0, 2, 1, 2, 0] and cols.dtype == torch.int32 and vals.tolist() == [2.0, 3.0, 2.0, 2.0, 5.0]
    rc, rp, cols, vals = dense_csr(dense, thr, "not_self")
    assert rp.tolist() == [0, 1, 2, 3, 3, 3, 3] and cols.tolist() == [2, 2, 0] and vals.tolist() == [3.0, 2.0, 5.0]
    rc, rp, cols, vals = dense_csr(dense, thr, "lower")
    assert rp.tolist() == [0, 0, 0, 1, 1, 1, 1] and cols.tolist() == [0] and vals.tolist() == [5.0]
    rc, rp, cols, vals = dense_csr(dense, torch.tensor([-inf, 9.0]), "lower")
    assert rc.tolist() == [[0, 1, 1], [0, 1, 2]] and cols.tolist() == [0, 0, 0, 0, 1]            # NaN at [0, 2, 1] stays out
    assert torch.equal(dense_mask(dense, thr, "all")[1], torch.zeros(3, 3, dtype=torch.bool))
    assert csr_of_mask(dense, torch.zeros_like(dense, dtype=torch.bool))[1].tolist() == [0] * 7
