"""Top-k screening over a checkpoint ensemble (mdg_bilinear_ensemble_topk, ops.bilinear_ensemble_topk, pipeline.ensemble_top_partners /
ensemble_top_pairs): what is decided without a GPU -- the C ABI as the header declares it, the workspace query, and the argument
checks that return before any launch (null pointers throughout: a launch would be an error of its own)."""
import ctypes

import pytest
import torch

NEW = ("mdg_bilinear_ensemble_topk", "mdg_bilinear_ensemble_topk_workspace_bytes")
PREC_F32, PREC_BF16X3, PREC_BF16 = 0, 1, 2
ALL, NOT_SELF, LOWER = 0, 1, 2


def test_the_library_exports_the_symbols_with_the_header_prototypes():
    from madrigal_amd import _lib
    L = _lib.lib()
    protos = _lib.declared_prototypes()
    for s in NEW + ("mdg_bilinear_ensemble_topk_chunk_tiles",):
        assert s in _lib.declared_symbols() and hasattr(L, s)
        assert (getattr(L, s).restype, list(getattr(L, s).argtypes)) == (protos[s][0], protos[s][1])
    assert L.mdg_bilinear_ensemble_topk.restype is ctypes.c_int and len(L.mdg_bilinear_ensemble_topk.argtypes) == 18
    assert L.mdg_bilinear_ensemble_topk_workspace_bytes.restype is ctypes.c_size_t
    assert L.mdg_abi_version() >= 25
    assert L.mdg_bilinear_ensemble_topk_chunk_tiles() >= 1


@pytest.mark.parametrize("sizes", [(4096, 4096, 896), (129, 1001, 2), (1, 1, 1), (5, 0, 3)])
@pytest.mark.parametrize("K", [1, 5, 8])
def test_workspace_is_the_ensemble_sweeps(sizes, K):
    from madrigal_amd._lib import lib
    L = lib()
    nh, nt, nl = sizes
    assert L.mdg_bilinear_ensemble_topk_workspace_bytes(nh, nt, nl, 128, K, PREC_F32) == 0
    assert (L.mdg_bilinear_ensemble_topk_workspace_bytes(nh, nt, nl, 128, K, PREC_BF16X3)
            == L.mdg_bilinear_ensemble_sigmoid_workspace_bytes(nh, nt, nl, 128, K, PREC_BF16X3))


def _call(n_models=2, k=4, prec=PREC_F32, eligible=ALL, nh=8, nt=8, D=128):
    from madrigal_amd._lib import lib
    return lib().mdg_bilinear_ensemble_topk(None, None, None, n_models, None, None, nh, nt, 2, D, prec, k, eligible, None, 0, None, None, 0)


@pytest.mark.parametrize("kw,word", [({"n_models": 0}, b"n_models"), ({"n_models": 9}, b"n_models"), ({"k": 0}, b"k must be"),
                                     ({"k": 33}, b"k must be"), ({"prec": PREC_BF16}, b"not offered"),
                                     ({"eligible": NOT_SELF, "nt": 9}, b"one drug set against itself"), ({"D": 64}, b"D must be")])
def test_bad_arguments_are_refused_before_any_launch(kw, word):
    from madrigal_amd._lib import lib
    assert _call(**kw) == -1
    msg = lib().mdg_last_error()
    assert b"mdg_bilinear_ensemble_topk" in msg and word in msg, msg


def test_good_arguments_with_null_pointers_stop_at_the_pointer_check_and_empty_sizes_pass():
    from madrigal_amd._lib import lib
    assert _call() == -1 and b"null pointer" in lib().mdg_last_error()
    assert _call(nh=0, nt=0) == 0


def _inputs(K, n=5, L=3):
    g = torch.Generator().manual_seed(0)
    return [torch.randn(n, 128, generator=g) for _ in range(K)], [torch.randn(L, 128, 128, generator=g) for _ in range(K)]


def test_ops_refuses_mismatched_lists_cpu_tensors_and_bad_k():
    from madrigal_amd import ops
    z, w = _inputs(2)
    with pytest.raises(ValueError, match="2 z_heads, 1 z_tails"):
        ops.bilinear_ensemble_topk(z, z[:1], w, 4)
    with pytest.raises(ValueError, match="2 z_heads, 2 z_tails, 1 w_syms"):
        ops.bilinear_ensemble_topk(z, z, w[:1], 4)
    with pytest.raises(ValueError, match="1..8"):
        ops.bilinear_ensemble_topk([], [], [], 4)
    with pytest.raises(ValueError, match="GPU"):
        ops.bilinear_ensemble_topk(z, z, w, 4)
    with pytest.raises(ValueError, match="precision"):
        ops.bilinear_ensemble_topk(z, z, w, 4, precision="bf16")
    with pytest.raises(ValueError, match="eligible"):
        ops.bilinear_ensemble_topk(z, z, w, 4, eligible="upper")


@pytest.mark.parametrize("kw", [{"K": 0}, {"K": True}, {"K": 2.0}, {"K": 10, "k_row": 0}, {"K": 10, "k_row": 33}, {"K": 10, "k_row": 2.0}])
def test_ensemble_top_pairs_validates_K_and_k_row_as_top_pairs_does(kw):
    from madrigal_amd import pipeline
    z, w = _inputs(2)
    with pytest.raises(ValueError, match="k_row" if "k_row" in kw else "K: expected"):
        pipeline.ensemble_top_pairs(w, z, **kw)


def test_the_pipeline_functions_refuse_bad_model_counts_and_cpu_embeddings():
    from madrigal_amd import pipeline
    z, w = _inputs(2)
    for fn, arg in ((pipeline.ensemble_top_partners, 4), (pipeline.ensemble_top_pairs, 10)):
        with pytest.raises(ValueError, match="1..8"):
            fn(w, z[:1], arg)
        with pytest.raises(ValueError, match="GPU"):
            fn(w, z, arg)
