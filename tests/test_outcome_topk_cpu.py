"""CPU checks of the streaming per-pair top-k over outcomes: the dense reference of the GPU tests reproduces the notebook's
np.partition reduction, ops.outcome_topk_merge of two states over disjoint outcome sets equals the reference over the union,
ops.outcome_topk refuses CPU tensors and bad k, and mdg_outcome_topk_update is declared, typed and exported and refuses bad
arguments before it touches a device."""
import ctypes

import numpy as np
import pytest
import torch

from outcome_topk_ref import INF, outcome_topk_ref, same_state

NEW = "mdg_outcome_topk_update"


def test_reference_is_the_notebooks_partition_reduction():
    """For random lists with ties the reference's k = 5 values are np.sort(np.partition(lst, len(lst)-5)[-5:])[::-1] exactly, its
    mean is the notebook's np.mean(...) within 1e-6 relative, and the ids attain the values, lowest outcome first among ties."""
    rng = np.random.default_rng(0)
    for L in (5, 6, 23, 158):
        x = (rng.integers(0, 12, size=(L, 9, 7)) / 12.0).astype(np.float32)          # rank-like values shared between outcomes
        x[:, 0, 0] = rng.standard_normal(L).astype(np.float32)                        # one list without ties
        vals, idx = outcome_topk_ref(torch.from_numpy(x), 5)
        assert vals.shape == (5, 9, 7) and idx.dtype == torch.int32
        for i in range(9):
            for j in range(7):
                lst = x[:, i, j]
                want = np.sort(np.partition(lst, len(lst) - 5)[-5:])[::-1]
                assert np.array_equal(vals[:, i, j].numpy(), want), (L, i, j)
                mean = float(np.mean(np.partition(lst, len(lst) - 5)[-5:]))
                assert abs(float(vals[:, i, j].mean()) - mean) <= 1e-6 * abs(mean), (L, i, j)
                ids = idx[:, i, j].tolist()
                assert np.array_equal(lst[ids], want) and len(set(ids)) == 5
                assert all(a < b for a, b, va, vb in zip(ids, ids[1:], want, want[1:]) if va == vb)
    low = outcome_topk_ref(torch.from_numpy(x), 5, largest=False)                     # the lowest five (fig5 :2050)
    assert np.array_equal(low[0][:, 3, 4].numpy(), np.sort(x[:, 3, 4])[:5])


def _tied(L, seed, nh=6, nt=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 4, (L, nh, nt), generator=g).float()          # almost every slot is decided by the outcome id
    x[0, 1, 2] = float("nan")
    x[L - 1, 2, 3] = -INF
    x[L // 2, 0, 0] = INF
    return x


@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("k", [1, 5, 8])
def test_merge_of_two_states_over_disjoint_outcomes_is_the_reference_over_the_union(k, largest):
    from madrigal_amd.ops import outcome_topk_merge
    x = _tied(11, 1)
    whole = outcome_topk_ref(x, k, largest=largest)
    labels = torch.arange(11)
    for pick in (labels < 4, labels % 2 == 0, labels >= 9, labels < 11, (labels == 3) | (labels == 7)):          # interleaved sets, short states, an empty side
        a = outcome_topk_ref(x[pick], k, labels=labels[pick], largest=largest)
        b = outcome_topk_ref(x[~pick], k, labels=labels[~pick], largest=largest)
        before = [t.clone() for t in a + b]
        for first, second in ((a, b), (b, a)):
            got = outcome_topk_merge(first, second, largest=largest)
            assert same_state(got, whole), (k, largest, pick.tolist())
        assert all(torch.equal(t, u) for t, u in zip(a + b, before))              # the arguments are left alone
    if k == 8:
        a = outcome_topk_ref(x[:3], k, largest=largest)                             # both states keep empty slots
        b = outcome_topk_ref(x[3:5], k, label_base=3, largest=largest)
        got = outcome_topk_merge(a, b, largest=largest)
        assert same_state(got, outcome_topk_ref(x[:5], k, largest=largest)) and bool((got[1][5:] == -1).all())
    with pytest.raises(ValueError, match="one shape"):
        outcome_topk_merge(outcome_topk_ref(x, 3), outcome_topk_ref(x, 4))


def test_wrapper_validation_without_a_gpu():
    from madrigal_amd import ops
    x = torch.zeros(3, 4, 4)
    for k in (0, 9, -1, 2.0, True):
        with pytest.raises(ValueError, match="k: expected an int in 1..8"):
            ops.outcome_topk(x, k)
    with pytest.raises(ValueError, match="GPU"):                      # a well-formed call on CPU tensors: no CPU fallback
        ops.outcome_topk(x, 5)
    with pytest.raises(ValueError, match="GPU"):
        ops.outcome_topk(x.half(), 5, labels=[0, 1, 2], largest=False, eligible="lower")


def test_symbol_is_declared_typed_and_exported():
    from madrigal_amd import _lib
    L = _lib.lib()
    assert NEW in _lib.declared_symbols() and hasattr(L, NEW) and L.mdg_abi_version() >= 24
    P, I, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert _lib.declared_prototypes()[NEW] == (I, [P, I, I64, I64, P, I64, P, P, P, P, I64, I64, I64, I64, I64, I, I, I, I, P])
    header = " ".join(open(_lib.HEADER).read().split())
    assert "fig5_t2d_mash.ipynb:1442-1448" in header and ":2034-2039" in header


def test_c_entry_refuses_bad_arguments_before_it_touches_a_device():
    from madrigal_amd._lib import lib
    L = lib()

    def f(x_type=0, ldx=4, lds=4, ss=16, nh=4, nt=4, nl=1, k=5, fresh=1, largest=1, eligible=0, base=0):
        return L.mdg_outcome_topk_update(None, x_type, 16, ldx, None, base, None, None, None, None, ss, lds, nh, nt, nl, k, fresh, largest, eligible, None)

    for kw, what in ((dict(x_type=3), b"x_type"), (dict(k=0), b"k = 0"), (dict(k=9), b"k = 9"), (dict(eligible=1), b"eligible"),
                     (dict(largest=2), b"largest"), (dict(nl=-1), b"negative size"), (dict(base=2 ** 31 - 1), b"int32 range"),
                     (dict(), b"null state")):
        assert f(**kw) == -1 and NEW.encode() in L.mdg_last_error() and what in L.mdg_last_error(), (kw, L.mdg_last_error())
    assert f(nh=0) == 0 and f(nt=0) == 0 and f(nl=0, fresh=0) == 0          # nothing to do
