"""Checkpoint-ensemble spread (mdg_bilinear_ensemble_spread / _spread_topk, ops.bilinear_ensemble_spread / _spread_topk,
pipeline.ensemble_spread_all_pairs / ensemble_confident_partners): what is decided without a GPU.

The recurrence: ``spread_ref.welford32`` restates the kernel's spread_update / spread_finish step by step in np.float32.  Its largest
absolute std error against float64 over ``spread_ref.cases()`` -- uniform probabilities and probabilities that round to 1, K = 2,
5, 8 -- is recorded as ``spread_ref.E_R``; the GPU test's tolerance is built on it.  The restatement must stay within 2 E_R, be
exactly 0 for equal values and K = 1, and the naive sum p^2 - (sum p)^2 / K must miss 2 E_R on the saturated inputs (it returns
noise of a few 1e-4 there, or NaN): the check has teeth.

The C ABI as the header declares it, the workspace query and the argument checks that return before any launch (null pointers
throughout); the wrappers' ValueErrors as far as they are raised before a device is needed."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import spread_ref as R

NEW = ("mdg_bilinear_ensemble_spread", "mdg_bilinear_ensemble_spread_topk", "mdg_bilinear_ensemble_spread_workspace_bytes",
       "mdg_bilinear_ensemble_spread_chunk_tiles")
PREC_F32, PREC_BF16X3, PREC_BF16 = 0, 1, 2
ALL, NOT_SELF, LOWER = 0, 1, 2


# ---- the recurrence ------------------------------------------------------------------------------------------------------------
def test_the_restatement_stays_within_twice_its_recorded_error_and_the_naive_formula_does_not():
    worst = 0.0
    for name, p in R.cases().items():
        e_w, e_n = R.std_error(R.welford32, p), R.std_error(R.naive32, p)
        noise = float(np.abs(np.nan_to_num(R.naive32(p)).astype(np.float64) - R.spread64(p)[1]).max())
        print(f"{name}: welford32 {e_w:.3e}, naive32 {e_n:.3e} (NaN as 0: {noise:.3e})")
        worst = max(worst, e_w)
        assert e_w <= 2 * R.E_R, name
        if name.startswith("saturated"):
            assert e_n > 2 * R.E_R and noise > 2 * R.E_R, name
        mean, std, m2 = R.welford32(p)
        assert bool((m2 >= 0).all()) and bool((std >= 0).all()) and not bool(np.isnan(std).any())
        s = p[0].copy()                                  # the mean is the running sum's: summed in model order, divided once
        for m in range(1, p.shape[0]):
            s = s + p[m]
        assert np.array_equal(mean, s / np.float32(p.shape[0]))
    print(f"largest: {worst:.4e} (E_R = {R.E_R:.4e})")
    assert R.E_R <= 1.01 * worst                         # the constant is the measurement, not a loosened bound


@pytest.mark.parametrize("K", [1, 2, 3, 5, 7, 8])
def test_equal_values_and_one_model_give_exactly_zero(K):
    rng = np.random.default_rng(K)
    one = np.concatenate([rng.random(4096).astype(np.float32), np.float32([0.0, 1.0, 1e-38, 1 - 2.0 ** -24])])
    mean, std, m2 = R.welford32(np.stack([one] * K))
    assert not m2.any() and not std.any()
    assert np.array_equal(std, np.zeros_like(std)) and not np.signbit(std).any()
    if K == 1:
        assert np.array_equal(mean, one)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_symbols_with_the_header_prototypes():
    from madrigal_amd import _lib
    L = _lib.lib()
    protos = _lib.declared_prototypes()
    for s in NEW:
        assert s in _lib.declared_symbols() and hasattr(L, s)
        assert (getattr(L, s).restype, list(getattr(L, s).argtypes)) == (protos[s][0], protos[s][1])
    assert L.mdg_bilinear_ensemble_spread.restype is ctypes.c_int and len(L.mdg_bilinear_ensemble_spread.argtypes) == 17
    assert L.mdg_bilinear_ensemble_spread.argtypes[7] is ctypes.c_float                    # kappa
    assert L.mdg_bilinear_ensemble_spread_topk.restype is ctypes.c_int and len(L.mdg_bilinear_ensemble_spread_topk.argtypes) == 21
    assert L.mdg_bilinear_ensemble_spread_topk.argtypes[4] is ctypes.c_float
    assert L.mdg_bilinear_ensemble_spread_workspace_bytes.restype is ctypes.c_size_t
    assert 1 <= L.mdg_bilinear_ensemble_spread_chunk_tiles() <= L.mdg_bilinear_ensemble_topk_chunk_tiles()


@pytest.mark.parametrize("sizes", [(4096, 4096, 896), (129, 1001, 2), (1, 1, 1), (5, 0, 3)])
@pytest.mark.parametrize("K", [1, 5, 8])
def test_workspace_is_the_ensemble_sweeps(sizes, K):
    from madrigal_amd._lib import lib
    L = lib()
    nh, nt, nl = sizes
    assert L.mdg_bilinear_ensemble_spread_workspace_bytes(nh, nt, nl, 128, K, PREC_F32) == 0
    assert (L.mdg_bilinear_ensemble_spread_workspace_bytes(nh, nt, nl, 128, K, PREC_BF16X3)
            == L.mdg_bilinear_ensemble_sigmoid_workspace_bytes(nh, nt, nl, 128, K, PREC_BF16X3))


def _dense(n_models=2, kappa=0.0, prec=PREC_F32, nh=8, nt=8, ldo=8, D=128):
    from madrigal_amd._lib import lib
    return lib().mdg_bilinear_ensemble_spread(None, None, None, n_models, None, None, None, kappa, ldo, nh, nt, 2, D, prec, None, 0, None)


def _topk(n_models=2, kappa=0.0, k=4, prec=PREC_F32, eligible=ALL, nh=8, nt=8, D=128):
    from madrigal_amd._lib import lib
    return lib().mdg_bilinear_ensemble_spread_topk(None, None, None, n_models, kappa, None, None, None, None, nh, nt, 2, D, prec, k, eligible,
                                                   None, 0, None, None, 0)


@pytest.mark.parametrize("kw,word", [({"n_models": 0}, b"n_models"), ({"n_models": 9}, b"n_models"), ({"prec": PREC_BF16}, b"not offered"),
                                     ({"D": 64}, b"D must be"), ({"ldo": 7}, b"row pitch"), ({"ldo": 1 << 22}, b"too large"),
                                     ({"kappa": float("nan")}, b"kappa"), ({"kappa": float("inf")}, b"kappa"),
                                     ({"kappa": float("-inf")}, b"kappa")])
def test_the_dense_entry_point_refuses_bad_arguments_before_any_launch(kw, word):
    from madrigal_amd._lib import lib
    assert _dense(**kw) == -1
    msg = lib().mdg_last_error()
    assert b"mdg_bilinear_ensemble_spread:" in msg and word in msg, msg


@pytest.mark.parametrize("kw,word", [({"n_models": 0}, b"n_models"), ({"n_models": 9}, b"n_models"), ({"k": 0}, b"k must be"),
                                     ({"k": 33}, b"k must be"), ({"prec": PREC_BF16}, b"not offered"),
                                     ({"eligible": NOT_SELF, "nt": 9}, b"one drug set against itself"), ({"D": 64}, b"D must be"),
                                     ({"kappa": float("nan")}, b"kappa"), ({"kappa": float("inf")}, b"kappa")])
def test_the_topk_entry_point_refuses_bad_arguments_before_any_launch(kw, word):
    from madrigal_amd._lib import lib
    assert _topk(**kw) == -1
    msg = lib().mdg_last_error()
    assert b"mdg_bilinear_ensemble_spread_topk" in msg and word in msg, msg


def test_good_arguments_with_null_pointers_stop_at_the_pointer_check_and_empty_sizes_pass():
    from madrigal_amd._lib import lib
    assert _dense() == -1 and b"null pointer" in lib().mdg_last_error()
    assert _topk() == -1 and b"null pointer" in lib().mdg_last_error()
    assert _dense(nh=0, nt=0, ldo=0) == 0 and _topk(nh=0, nt=0) == 0


# ---- the wrappers ----------------------------------------------------------------------------------------------------------------
def _inputs(K, n=5, L=3):
    g = torch.Generator().manual_seed(0)
    return [torch.randn(n, 128, generator=g) for _ in range(K)], [torch.randn(L, 128, 128, generator=g) for _ in range(K)]


@pytest.mark.parametrize("kappa", [float("nan"), float("inf"), float("-inf"), np.float32("nan"), 1e39, "1", None, True, 1j])
def test_ops_refuses_a_kappa_that_is_not_a_finite_real(kappa):
    from madrigal_amd import ops
    z, w = _inputs(2)
    with pytest.raises(ValueError, match="kappa"):
        ops.bilinear_ensemble_spread_topk(z, z, w, 4, kappa)
    if kappa is not None:                                 # None: the dense product without a bound
        with pytest.raises(ValueError, match="kappa"):
            ops.bilinear_ensemble_spread(z, z, w, kappa=kappa)


@pytest.mark.parametrize("kappa", [-1, 0.5, np.float32(-2.0), np.float64(0.0), np.int64(3)])
def test_ops_accepts_python_and_numpy_reals_and_then_asks_for_a_gpu(kappa):
    from madrigal_amd import ops
    z, w = _inputs(2)
    with pytest.raises(ValueError, match="GPU"):
        ops.bilinear_ensemble_spread_topk(z, z, w, 4, kappa)
    with pytest.raises(ValueError, match="GPU"):
        ops.bilinear_ensemble_spread(z, z, w, kappa=kappa)


@pytest.mark.parametrize("k", [0, 33, -1, 2.0, True, None])
def test_ops_refuses_a_bad_k(k):
    from madrigal_amd import ops
    z, w = _inputs(2)
    with pytest.raises(ValueError, match="k: expected"):
        ops.bilinear_ensemble_spread_topk(z, z, w, k, -1.0)


def test_ops_refuses_mismatched_lists_and_unknown_names():
    from madrigal_amd import ops
    z, w = _inputs(2)
    for fn in (lambda *a, **kw: ops.bilinear_ensemble_spread(*a, **kw), lambda *a, **kw: ops.bilinear_ensemble_spread_topk(*a, 4, -1.0, **kw)):
        with pytest.raises(ValueError, match="2 z_heads, 1 z_tails"):
            fn(z, z[:1], w)
        with pytest.raises(ValueError, match="1..8"):
            fn([], [], [])
        with pytest.raises(ValueError, match="precision"):
            fn(z, z, w, precision="bf16")
        with pytest.raises(ValueError, match="GPU"):
            fn(z, z, w)
    with pytest.raises(ValueError, match="eligible"):
        ops.bilinear_ensemble_spread_topk(z, z, w, 4, -1.0, eligible="upper")
    with pytest.raises(ValueError, match="one drug set"):
        ops.bilinear_ensemble_spread_topk(z, [t[:3] for t in z], w, 4, -1.0, eligible="lower")


def test_ops_refuses_an_out_tuple_of_the_wrong_shape():
    from madrigal_amd import ops
    z, w = _inputs(2)                                     # L = 3, N = 5
    f = lambda *s: torch.zeros(s)                         # noqa: E731
    i = lambda *s: torch.zeros(s, dtype=torch.int32)      # noqa: E731
    with pytest.raises(ValueError, match=r"out: expected a \(mean, std\) tuple"):
        ops.bilinear_ensemble_spread(z, z, w, out=(f(3, 5, 5), f(3, 5, 5), f(3, 5, 5)))
    with pytest.raises(ValueError, match=r"out: expected a \(mean, std, bound\) tuple"):
        ops.bilinear_ensemble_spread(z, z, w, kappa=1.0, out=(f(3, 5, 5), f(3, 5, 5)))
    with pytest.raises(ValueError, match=r"out \(std\)"):
        ops.bilinear_ensemble_spread(z, z, w, out=(f(3, 5, 5), f(3, 5, 6)))
    with pytest.raises(ValueError, match=r"out \(mean\)"):
        ops.bilinear_ensemble_spread(z, z, w, out=(f(3, 5, 5).double(), None))
    with pytest.raises(ValueError, match="at least one"):
        ops.bilinear_ensemble_spread(z, z, w, out=(None, None))
    with pytest.raises(ValueError, match="GPU"):          # a well-shaped tuple passes on to the device check
        ops.bilinear_ensemble_spread(z, z, w, out=(None, f(3, 5, 5)))
    with pytest.raises(ValueError, match=r"\(bound, idx, mean, std\)"):
        ops.bilinear_ensemble_spread_topk(z, z, w, 4, -1.0, out=(f(3, 5, 4), i(3, 5, 4)))
    with pytest.raises(ValueError, match=r"out\[0\]"):
        ops.bilinear_ensemble_spread_topk(z, z, w, 4, -1.0, out=(f(3, 5, 3), i(3, 5, 4), f(3, 5, 4), f(3, 5, 4)))
    with pytest.raises(ValueError, match=r"out\[1\]"):
        ops.bilinear_ensemble_spread_topk(z, z, w, 4, -1.0, out=(f(3, 5, 4), f(3, 5, 4), f(3, 5, 4), f(3, 5, 4)))
    with pytest.raises(ValueError, match=r"out\[3\]"):
        ops.bilinear_ensemble_spread_topk(z, z, w, 4, -1.0, out=(f(3, 5, 4), i(3, 5, 4), f(3, 5, 4), f(3, 5, 8)[:, :, ::2]))


def test_the_pipeline_functions_refuse_bad_model_counts_and_cpu_embeddings():
    from madrigal_amd import pipeline
    z, w = _inputs(2)
    for fn in (lambda *a, **kw: pipeline.ensemble_spread_all_pairs(*a, **kw), lambda *a, **kw: pipeline.ensemble_confident_partners(*a, 4, **kw)):
        with pytest.raises(ValueError, match="1..8"):
            fn(w, z[:1])
        with pytest.raises(ValueError, match="GPU"):
            fn(w, z)
    sig = inspect.signature(pipeline.ensemble_confident_partners)
    assert sig.parameters["kappa"].default == -1.0 and sig.parameters["eligible"].default == "not_self"     # mean - std over j != i
