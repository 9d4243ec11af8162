"""Threshold selection over a checkpoint ensemble (mdg_bilinear_ensemble_select_count / _fill, ops.bilinear_ensemble_select_count /
bilinear_ensemble_select, pipeline.ensemble_partner_counts / ensemble_partners_above / ensemble_pairs_above): what is decided without
a GPU -- the C ABI as the header declares it, the workspace query, and the argument checks that return before any launch (null
pointers throughout: a launch would be an error of its own)."""
import ctypes

import pytest
import torch

NEW = ("mdg_bilinear_ensemble_select_workspace_bytes", "mdg_bilinear_ensemble_select_count", "mdg_bilinear_ensemble_select_fill")
PREC_F32, PREC_BF16X3, PREC_BF16, PREC_F16 = 0, 1, 2, 3
ALL, NOT_SELF, LOWER = 0, 1, 2


def test_the_library_exports_the_symbols_with_the_header_prototypes():
    from madrigal_amd import _lib
    L = _lib.lib()
    protos = _lib.declared_prototypes()
    for s in NEW:
        assert s in _lib.declared_symbols() and hasattr(L, s)
        assert (getattr(L, s).restype, list(getattr(L, s).argtypes)) == (protos[s][0], protos[s][1])
    I, I64, Z, P = ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_void_p
    assert protos[NEW[0]] == (Z, [I64, I64, I64, I64, I, I])
    assert protos[NEW[1]] == (I, [P, P, P, I, P, P, I64, I64, I64, I64, I, I, P, Z, P, P, I64])
    assert protos[NEW[2]] == (I, [P, P, P, I, P, P, P, P, I64, I64, I64, I64, I, I, P, Z, P, P, I64])
    assert L.mdg_abi_version() >= 26


@pytest.mark.parametrize("sizes", [(4096, 4096, 896), (129, 1001, 2), (1, 1, 1), (5, 0, 3)])
@pytest.mark.parametrize("K", [1, 5, 8])
def test_workspace_is_the_ensemble_sweeps(sizes, K):
    from madrigal_amd._lib import lib
    L = lib()
    nh, nt, nl = sizes
    assert L.mdg_bilinear_ensemble_select_workspace_bytes(nh, nt, nl, 128, K, PREC_F32) == 0
    assert (L.mdg_bilinear_ensemble_select_workspace_bytes(nh, nt, nl, 128, K, PREC_BF16X3)
            == L.mdg_bilinear_ensemble_sigmoid_workspace_bytes(nh, nt, nl, 128, K, PREC_BF16X3))
    assert L.mdg_bilinear_ensemble_select_workspace_bytes(nh, nt, nl, 128, 0, PREC_BF16X3) == 0


def _count(n_models=2, prec=PREC_F32, eligible=ALL, nh=8, nt=8, nl=2, D=128):
    from madrigal_amd._lib import lib
    return lib().mdg_bilinear_ensemble_select_count(None, None, None, n_models, None, None, nh, nt, nl, D, prec, eligible, None, 0, None, None, 0)


def _fill(n_models=2, prec=PREC_F32, eligible=ALL, nh=8, nt=8, nl=2, D=128):
    from madrigal_amd._lib import lib
    return lib().mdg_bilinear_ensemble_select_fill(None, None, None, n_models, None, None, None, None, nh, nt, nl, D, prec, eligible, None, 0,
                                                   None, None, 0)


ENTRIES = [(_count, b"mdg_bilinear_ensemble_select_count"), (_fill, b"mdg_bilinear_ensemble_select_fill")]


@pytest.mark.parametrize("entry", ENTRIES, ids=["count", "fill"])
@pytest.mark.parametrize("kw,word", [({"n_models": 0}, b"n_models"), ({"n_models": 9}, b"n_models"), ({"prec": PREC_BF16}, b"not offered"),
                                     ({"prec": PREC_F16}, b"not offered"), ({"prec": 7}, b"precision"),
                                     ({"eligible": NOT_SELF, "nt": 9}, b"one drug set against itself"),
                                     ({"eligible": LOWER, "nt": 9}, b"one drug set against itself"), ({"eligible": 9}, b"eligible"),
                                     ({"D": 64}, b"D must be"), ({"nl": 65536}, b"n_labels"), ({"nh": -1}, b"negative"),
                                     ({"nt": (1 << 31) - 64}, b"int32 column indices"), ({"nt": 0}, b"n_tail must be at least 1")])
def test_bad_arguments_are_refused_before_any_launch(entry, kw, word):
    from madrigal_amd._lib import lib
    fn, name = entry
    assert fn(**kw) == -1
    msg = lib().mdg_last_error()
    assert name in msg and word in msg, msg


@pytest.mark.parametrize("entry", ENTRIES, ids=["count", "fill"])
def test_good_arguments_with_null_pointers_stop_at_the_pointer_check_and_empty_sizes_pass(entry):
    from madrigal_amd._lib import lib
    fn, name = entry
    assert fn() == -1 and name in lib().mdg_last_error() and b"null pointer" in lib().mdg_last_error()
    assert fn(nh=0) == 0
    assert fn(nh=0, nt=0) == 0
    assert fn(nl=0) == 0


def test_null_model_pointers_and_the_workspace_are_checked_per_model():
    """Non-null host arrays whose entries are null; then (aligned, never dereferenced) made-up addresses with no workspace."""
    from madrigal_amd._lib import lib
    L = lib()
    null = (ctypes.c_void_p * 2)(None, None)
    some = ctypes.c_void_p(4096)
    assert L.mdg_bilinear_ensemble_select_count(null, null, null, 2, some, some, 8, 8, 2, 128, PREC_F32, ALL, None, 0, None, None, 0) == -1
    assert b"mdg_bilinear_ensemble_select_count: null pointer for model 0" in L.mdg_last_error()
    odd = (ctypes.c_void_p * 2)(4096, 4100)
    assert L.mdg_bilinear_ensemble_select_fill(odd, odd, odd, 2, some, some, some, some, 8, 8, 2, 128, PREC_F32, ALL, None, 0, None, None, 0) == -1
    assert b"mdg_bilinear_ensemble_select_fill" in L.mdg_last_error() and b"16-byte aligned (model 1)" in L.mdg_last_error()
    ok = (ctypes.c_void_p * 2)(4096, 8192)
    for fn, extra in ((L.mdg_bilinear_ensemble_select_count, (some,)), (L.mdg_bilinear_ensemble_select_fill, (some, some, some))):
        assert fn(ok, ok, ok, 2, some, *extra, 8, 8, 2, 128, PREC_BF16X3, ALL, None, 0, None, None, 0) == -2      # MDG_EWORKSPACE
        assert b"mdg_bilinear_ensemble_select_" in L.mdg_last_error() and b"workspace" in L.mdg_last_error()


def _inputs(K, n=5, L=3):
    g = torch.Generator().manual_seed(0)
    return [torch.randn(n, 128, generator=g) for _ in range(K)], [torch.randn(L, 128, 128, generator=g) for _ in range(K)]


def test_ops_refuses_mismatched_lists_bad_names_bad_thresholds_and_cpu_tensors():
    from madrigal_amd import ops
    z, w = _inputs(2)
    thr = torch.full((3,), 0.5)
    for f in (ops.bilinear_ensemble_select_count, ops.bilinear_ensemble_select):
        with pytest.raises(ValueError, match="2 z_heads, 1 z_tails"):
            f(z, z[:1], w, thr)
        with pytest.raises(ValueError, match="2 z_heads, 2 z_tails, 1 w_syms"):
            f(z, z, w[:1], thr)
        with pytest.raises(ValueError, match="1..8"):
            f([], [], [], thr)
        with pytest.raises(ValueError, match="1..8"):
            f((z * 5)[:9], (z * 5)[:9], (w * 5)[:9], thr)   # list repetition: nine models
        with pytest.raises(ValueError, match="precision"):
            f(z, z, w, thr, precision="bf16")
        with pytest.raises(ValueError, match="eligible"):
            f(z, z, w, thr, eligible="upper")
        with pytest.raises(ValueError, match="one cut per outcome"):
            f(z, z, w, torch.zeros(4))
        with pytest.raises(ValueError, match="NaN"):
            f(z, z, w, torch.tensor([0.5, float("nan"), 0.5]))
        with pytest.raises(ValueError, match="one drug set"):
            f(z, [t[:4] for t in z], w, thr, eligible="lower")
        with pytest.raises(ValueError, match="model 1 has"):
            f(z, z, [w[0], w[1][:2]], thr)
        with pytest.raises(ValueError, match="GPU"):
            f(z, z, w, thr)


def test_the_pipeline_functions_refuse_bad_model_counts_and_cpu_embeddings():
    from madrigal_amd import pipeline
    z, w = _inputs(2)
    for fn in (pipeline.ensemble_partner_counts, pipeline.ensemble_partners_above, pipeline.ensemble_pairs_above):
        with pytest.raises(ValueError, match="1..8"):
            fn(w, z[:1], 0.9)
        with pytest.raises(ValueError, match="1..8"):
            fn([], [], 0.9)
        with pytest.raises(ValueError, match="1..8"):
            fn((w * 5)[:9], (z * 5)[:9], 0.9)
        with pytest.raises(ValueError, match="GPU"):
            fn(w, z, 0.9)
