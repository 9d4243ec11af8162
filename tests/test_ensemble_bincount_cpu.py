"""Counting the checkpoint ensemble's probabilities between edges (mdg_bilinear_ensemble_bincount / _split,
ops.bilinear_ensemble_bincount, pipeline.ensemble_score_histogram / ensemble_count_below / ensemble_normalized_ranks_of /
ensemble_recovery_at_cuts / ensemble_auroc_bounds): what is decided without a GPU -- the C ABI as the header declares it, the workspace
query, and the argument checks that return before any launch (null or made-up pointers throughout: a launch would be an error of its
own)."""
import ctypes

import pytest
import torch

NEW = ("mdg_bilinear_ensemble_bincount_workspace_bytes", "mdg_bilinear_ensemble_bincount", "mdg_bilinear_ensemble_bincount_split")
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
    assert protos[NEW[1]] == (I, [P, P, P, I, P, P, I64, I64, I64, I64, I, I, I, P, Z, P])
    assert protos[NEW[2]] == (I, [P, P, P, I, P, P, I64, I64, I64, I64, I, I, I, P, Z, P, P, I64])
    assert L.mdg_abi_version() >= 28


@pytest.mark.parametrize("sizes", [(4096, 4096, 896), (129, 1001, 2), (1, 1, 1), (5, 0, 3)])
@pytest.mark.parametrize("K", [1, 5, 8])
def test_workspace_is_the_ensemble_sweeps(sizes, K):
    from madrigal_amd._lib import lib
    L = lib()
    nh, nt, nl = sizes
    assert L.mdg_bilinear_ensemble_bincount_workspace_bytes(nh, nt, nl, 128, K, PREC_F32) == 0
    for prec in (PREC_F32, PREC_BF16X3):
        assert (L.mdg_bilinear_ensemble_bincount_workspace_bytes(nh, nt, nl, 128, K, prec)
                == L.mdg_bilinear_ensemble_sigmoid_workspace_bytes(nh, nt, nl, 128, K, prec))
    assert L.mdg_bilinear_ensemble_bincount_workspace_bytes(nh, nt, nl, 128, 0, PREC_BF16X3) == 0


def _plain(n_models=2, prec=PREC_F32, eligible=ALL, nh=8, nt=8, nl=2, D=128, n_edges=4):
    from madrigal_amd._lib import lib
    return lib().mdg_bilinear_ensemble_bincount(None, None, None, n_models, None, None, nh, nt, nl, D, n_edges, prec, eligible, None, 0, None)


def _split(n_models=2, prec=PREC_F32, eligible=ALL, nh=8, nt=8, nl=2, D=128, n_edges=4):
    from madrigal_amd._lib import lib
    return lib().mdg_bilinear_ensemble_bincount_split(None, None, None, n_models, None, None, nh, nt, nl, D, n_edges, prec, eligible, None, 0,
                                                      None, None, 0)


ENTRIES = [(_plain, b"mdg_bilinear_ensemble_bincount:"), (_split, b"mdg_bilinear_ensemble_bincount_split:")]


@pytest.mark.parametrize("entry", ENTRIES, ids=["plain", "split"])
@pytest.mark.parametrize("kw,word", [({"n_models": 0}, b"n_models"), ({"n_models": 9}, b"n_models"), ({"prec": PREC_BF16}, b"not offered"),
                                     ({"prec": PREC_F16}, b"not offered"), ({"prec": 7}, b"precision"), ({"D": 64}, b"D must be"),
                                     ({"n_edges": 0}, b"n_edges"), ({"n_edges": 1025}, b"n_edges"),
                                     ({"nh": 1 << 23, "nt": 1 << 23}, b"n_tail 8388608 does not fit"), ({"nt": 1 << 23}, b"n_tail 8388608 does not fit"),
                                     ({"eligible": NOT_SELF, "nt": 9}, b"one drug set against itself"),
                                     ({"eligible": LOWER, "nt": 9}, b"one drug set against itself"), ({"eligible": 9}, b"eligible"),
                                     ({"nl": 65536}, b"n_labels"), ({"nh": -1}, b"negative"), ({"nt": 0}, b"n_tail must be at least 1")])
def test_bad_arguments_are_refused_before_any_launch(entry, kw, word):
    from madrigal_amd._lib import lib
    fn, name = entry
    assert fn(**kw) == -1
    msg = lib().mdg_last_error()
    assert msg.startswith(name) and word in msg, msg


@pytest.mark.parametrize("entry", ENTRIES, ids=["plain", "split"])
def test_good_arguments_with_null_pointers_stop_at_the_pointer_check_and_empty_sizes_pass(entry):
    from madrigal_amd._lib import lib
    fn, name = entry
    assert lib().mdg_bilinear_bincount_max_edges() == 1024
    for kw in ({}, {"n_edges": 1}, {"n_edges": 1024}, {"nt": (1 << 23) - 1}, {"nl": 65535}, {"eligible": LOWER}, {"prec": PREC_BF16X3}):
        assert fn(**kw) == -1 and lib().mdg_last_error().startswith(name) and b"null pointer" in lib().mdg_last_error(), kw
    assert fn(nh=0) == 0               # (null counts: nothing to zero)
    assert fn(nh=0, nt=0) == 0
    assert fn(nl=0) == 0
    assert fn(nh=0, eligible=NOT_SELF) == -1          # the size rules hold for an empty call too


def test_null_model_pointers_alignment_the_workspace_and_the_mask_are_checked():
    """Non-null host arrays whose entries are null; then (never dereferenced) made-up addresses: misaligned operands, a missing, short
    and misaligned workspace, and the mask arguments of _split, all of which return before anything is enqueued."""
    from madrigal_amd._lib import lib
    L = lib()
    null = (ctypes.c_void_p * 2)(None, None)
    some = ctypes.c_void_p(4096)
    tail = (8, 8, 2, 128, 4)
    assert L.mdg_bilinear_ensemble_bincount(null, null, null, 2, some, some, *tail, PREC_F32, ALL, None, 0, None) == -1
    assert b"mdg_bilinear_ensemble_bincount: null pointer for model 0" in L.mdg_last_error()
    half = (ctypes.c_void_p * 2)(4096, None)
    assert L.mdg_bilinear_ensemble_bincount_split(half, half, half, 2, some, some, *tail, PREC_F32, ALL, None, 0, None, None, 0) == -1
    assert b"mdg_bilinear_ensemble_bincount_split: null pointer for model 1" in L.mdg_last_error()
    ok = (ctypes.c_void_p * 2)(4096, 8192)
    for edges, counts in ((None, some), (some, None)):
        assert L.mdg_bilinear_ensemble_bincount(ok, ok, ok, 2, edges, counts, *tail, PREC_F32, ALL, None, 0, None) == -1
        assert b"mdg_bilinear_ensemble_bincount: null pointer" in L.mdg_last_error()
    odd = (ctypes.c_void_p * 2)(4096, 4100)
    for lists in ((odd, ok, ok), (ok, odd, ok), (ok, ok, odd)):
        assert L.mdg_bilinear_ensemble_bincount(*lists, 2, some, some, *tail, PREC_F32, ALL, None, 0, None) == -1
        assert b"mdg_bilinear_ensemble_bincount:" in L.mdg_last_error() and b"16-byte aligned (model 1)" in L.mdg_last_error()
    need = L.mdg_bilinear_ensemble_bincount_workspace_bytes(8, 8, 2, 128, 2, PREC_BF16X3)
    assert need > 0
    for ws, nbytes in ((None, 0), (some, need - 1), (ctypes.c_void_p(4100), need), (None, need)):
        assert L.mdg_bilinear_ensemble_bincount(ok, ok, ok, 2, some, some, *tail, PREC_BF16X3, ALL, ws, nbytes, None) == -2      # MDG_EWORKSPACE
        assert b"mdg_bilinear_ensemble_bincount:" in L.mdg_last_error() and b"workspace" in L.mdg_last_error()
        assert L.mdg_bilinear_ensemble_bincount_split(ok, ok, ok, 2, some, some, *tail, PREC_BF16X3, ALL, ws, nbytes, None, some, 0) == -2
        assert b"mdg_bilinear_ensemble_bincount_split:" in L.mdg_last_error() and b"workspace" in L.mdg_last_error()
    split = lambda mask, stride: L.mdg_bilinear_ensemble_bincount_split(ok, ok, ok, 2, some, some, *tail, PREC_F32, ALL, None, 0, None,   # noqa: E731
                                                                         mask, stride)
    assert split(ctypes.c_void_p(4098), 0) == -1
    assert b"mdg_bilinear_ensemble_bincount_split: mask must be 4-byte aligned" in L.mdg_last_error()
    words = L.mdg_pair_mask_plane_words(8, 8)
    for stride in (5, words - 1, -1):
        assert split(some, stride) == -1
        assert b"mdg_bilinear_ensemble_bincount_split:" in L.mdg_last_error() and b"plane_stride" in L.mdg_last_error()


def _inputs(K, n=5, L=3):
    g = torch.Generator().manual_seed(0)
    return [torch.randn(n, 128, generator=g) for _ in range(K)], [torch.randn(L, 128, 128, generator=g) for _ in range(K)]


def test_ops_refuses_mismatched_lists_bad_names_bad_edges_and_cpu_tensors():
    from madrigal_amd import ops
    f = ops.bilinear_ensemble_bincount
    z, w = _inputs(2)
    e = torch.tensor([[0.25, 0.5]] * 3)
    with pytest.raises(ValueError, match="2 z_heads, 1 z_tails"):
        f(z, z[:1], w, e)
    with pytest.raises(ValueError, match="2 z_heads, 2 z_tails, 1 w_syms"):
        f(z, z, w[:1], e)
    with pytest.raises(ValueError, match="1..8"):
        f([], [], [], e)
    with pytest.raises(ValueError, match="1..8"):
        f((z * 5)[:9], (z * 5)[:9], (w * 5)[:9], e)   # list repetition: nine models
    with pytest.raises(ValueError, match="precision"):
        f(z, z, w, e, precision="bf16")
    with pytest.raises(ValueError, match="precision"):
        f(z, z, w, e, precision="f16")
    with pytest.raises(ValueError, match="eligible"):
        f(z, z, w, e, eligible="upper")
    with pytest.raises(ValueError, match="one row per outcome"):
        f(z, z, w, e[:2])
    with pytest.raises(ValueError, match="edges: expected a float32 tensor with 2 dims"):
        f(z, z, w, e[0])
    with pytest.raises(ValueError, match="edges: expected a float32 tensor with 2 dims"):
        f(z, z, w, e.double())
    with pytest.raises(ValueError, match="1..1024 edges"):
        f(z, z, w, torch.zeros(3, 0))
    with pytest.raises(ValueError, match="1..1024 edges"):
        f(z, z, w, torch.zeros(3, 1025))
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="finite"):
            f(z, z, w, torch.tensor([[0.25, 0.5], [0.25, bad], [0.25, 0.5]]))
    with pytest.raises(ValueError, match="ascending"):
        f(z, z, w, torch.tensor([[0.25, 0.5], [0.5, 0.25], [0.25, 0.5]]))
    with pytest.raises(ValueError, match="one drug set"):
        f(z, [t[:4] for t in z], w, e, eligible="lower")
    with pytest.raises(ValueError, match="model 1 has"):
        f(z, z, [w[0], w[1][:2]], e)
    with pytest.raises(ValueError, match="GPU"):
        f(z, z, w, e)
    with pytest.raises(ValueError, match="GPU"):
        f(z, z, w, e, split=torch.zeros((1, 1, 64), dtype=torch.int32))


def test_the_pipeline_functions_refuse_bad_model_counts_cpu_embeddings_and_a_known_that_is_no_mask():
    from madrigal_amd import pipeline
    z, w = _inputs(2)
    e = torch.tensor([0.25, 0.5])
    q = torch.full((3, 2), 0.5)
    known = torch.zeros((1, 1, 64), dtype=torch.int32)
    calls = {"ensemble_score_histogram": lambda m, zs, **kw: pipeline.ensemble_score_histogram(m, zs, e, **kw),
             "ensemble_count_below": lambda m, zs, **kw: pipeline.ensemble_count_below(m, zs, q, **kw),
             "ensemble_normalized_ranks_of": lambda m, zs: pipeline.ensemble_normalized_ranks_of(m, zs, q),
             "ensemble_recovery_at_cuts": lambda m, zs, known=known: pipeline.ensemble_recovery_at_cuts(m, zs, known, q),
             "ensemble_auroc_bounds": lambda m, zs, known=known: pipeline.ensemble_auroc_bounds(m, zs, known, e)}
    for name, fn in calls.items():
        with pytest.raises(ValueError, match="1..8"):
            fn(w, z[:1])
        with pytest.raises(ValueError, match="1..8"):
            fn([], [])
        with pytest.raises(ValueError, match="1..8"):
            fn((w * 5)[:9], (z * 5)[:9])
        with pytest.raises(ValueError, match="GPU"):
            fn(w, z)
        if name != "ensemble_normalized_ranks_of":
            for bad in ("drugs.csv", torch.zeros((1, 64), dtype=torch.int32), [[0, 1]]):
                with pytest.raises(ValueError, match="known: expected a mask"):
                    fn(w, z, known=bad)
    for name in ("ensemble_recovery_at_cuts", "ensemble_auroc_bounds"):
        with pytest.raises(ValueError, match="known: expected a mask"):
            calls[name](w, z, known=None)
