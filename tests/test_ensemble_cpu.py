"""Checkpoint-ensembled probabilities (ops.bilinear_ensemble_sigmoid, pipeline.ensemble_all_pairs): what is decided without a GPU --
the workspace query of the C ABI and the argument checks that run before any launch."""
import ctypes

import pytest
import torch


def test_workspace_query_answers_without_a_device():
    from madrigal_amd._lib import lib
    L = lib()
    q = lambda nh, nt, l, d, k, p: L.mdg_bilinear_ensemble_sigmoid_workspace_bytes(  # noqa: E731
        ctypes.c_int64(nh), ctypes.c_int64(nt), ctypes.c_int64(l), ctypes.c_int64(d), ctypes.c_int(k), ctypes.c_int(p))
    one = L.mdg_bilinear_allpairs_workspace_bytes(ctypes.c_int64(4096), ctypes.c_int64(4096), ctypes.c_int64(896), ctypes.c_int64(128), 1)
    assert q(4096, 4096, 896, 128, 1, 1) == one                  # one model: the head's own split-bf16 images
    assert q(4096, 4096, 896, 128, 5, 1) == 5 * one               # one set of images per checkpoint
    assert q(4096, 4096, 896, 128, 5, 0) == 0                     # exact fp32 reads the caller's tensors
    assert q(4096, 0, 896, 128, 5, 1) == 0


def test_bad_arguments_are_refused_by_the_library_without_a_launch():
    from madrigal_amd._lib import lib
    L = lib()
    arr = (ctypes.c_void_p * 9)(*([16] * 9))
    call = lambda k, ldo, nt, d, wsb: L.mdg_bilinear_ensemble_sigmoid(  # noqa: E731
        arr, arr, arr, ctypes.c_int(k), ctypes.c_void_p(16), ctypes.c_int64(ldo), ctypes.c_int64(8), ctypes.c_int64(nt),
        ctypes.c_int64(2), ctypes.c_int64(d), ctypes.c_int(1), ctypes.c_void_p(16), ctypes.c_size_t(wsb), ctypes.c_void_p(0))
    assert call(0, 8, 8, 128, 1 << 30) != 0 and b"n_models" in L.mdg_last_error()
    assert call(9, 8, 8, 128, 1 << 30) != 0 and b"n_models" in L.mdg_last_error()
    assert call(2, 8, 8, 64, 1 << 30) != 0 and b"D must be" in L.mdg_last_error()
    assert call(2, 7, 8, 128, 1 << 30) != 0 and b"row pitch" in L.mdg_last_error()
    assert call(2, 8, 8, 128, 16) != 0 and b"workspace" in L.mdg_last_error()


def _inputs(K, n=5, L=3, device="cpu"):
    g = torch.Generator().manual_seed(0)
    z = [torch.randn(n, 128, generator=g).to(device) for _ in range(K)]
    w = [torch.randn(L, 128, 128, generator=g).to(device) for _ in range(K)]
    return z, w


def test_ops_refuses_cpu_tensors_and_bad_model_counts():
    from madrigal_amd import ops
    z, w = _inputs(2)
    with pytest.raises(ValueError, match="GPU"):
        ops.bilinear_ensemble_sigmoid(z, z, w)
    with pytest.raises(ValueError, match="1..8"):
        ops.bilinear_ensemble_sigmoid([], [], [])
    z9, w9 = _inputs(9)
    with pytest.raises(ValueError, match="1..8"):
        ops.bilinear_ensemble_sigmoid(z9, z9, w9)
    with pytest.raises(ValueError):
        ops.bilinear_ensemble_sigmoid(z, z[:1], w)
    with pytest.raises(ValueError, match="precision"):
        ops.bilinear_ensemble_sigmoid(z, z, w, precision="bf16")


class _FakeCuda(torch.Tensor):
    """A CPU tensor that claims to live on the GPU: the shape checks run, no launch can follow on this machine."""

    @property
    def is_cuda(self):
        return True


def _fake(t):
    return t.as_subclass(_FakeCuda)


@pytest.mark.parametrize("what", ["L", "N", "D"])
def test_ops_refuses_mismatched_shapes(what):
    from madrigal_amd import ops
    z, w = _inputs(2)
    if what == "L":
        w[1] = w[1][:2]
    elif what == "N":
        z[1] = z[1][:4]
    else:
        z[1] = torch.randn(5, 64)
    with pytest.raises(ValueError, match="model 1"):
        ops.bilinear_ensemble_sigmoid([_fake(t) for t in z], [_fake(t) for t in z], [_fake(t) for t in w])


@pytest.mark.parametrize("kw", [{"drug_inds": [0, 5]}, {"drug_inds": [-1]}, {"drug_2_inds": [7]}, {"outcome_inds": [3]},
                                {"outcome_inds": [0, -2]}])
def test_pipeline_refuses_out_of_range_indices(kw, monkeypatch):
    from madrigal_amd import ops, pipeline
    z, w = _inputs(2)
    monkeypatch.setattr(ops, "symmetrize", lambda t: t)            # no launch: the weights are taken as they are
    with pytest.raises(ValueError, match="indices"):
        pipeline.ensemble_all_pairs(w, [_fake(t) for t in z], **kw)


def test_pipeline_refuses_bad_model_counts():
    from madrigal_amd import pipeline
    z, w = _inputs(2)
    with pytest.raises(ValueError, match="1..8"):
        pipeline.ensemble_all_pairs(w, z[:1])
    z9, w9 = _inputs(9)
    with pytest.raises(ValueError, match="1..8"):
        pipeline.ensemble_all_pairs(w9, z9)
    with pytest.raises(ValueError, match="GPU"):
        pipeline.ensemble_all_pairs(w, z)
