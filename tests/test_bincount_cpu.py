"""CPU checks of the counting product of the all-pairs head: the C ABI of mdg_bilinear_bincount is declared and exported, the
wrapper validates before it touches a device, and pipeline.ranks_from_counts restates the reference's rank arithmetic exactly."""
import pytest
import torch

from bincount_ref import brute_less, is_unique

NEW = ("mdg_bilinear_bincount", "mdg_bilinear_bincount_workspace_bytes", "mdg_bilinear_bincount_max_edges")


def test_bincount_symbols_are_declared_and_exported():
    from madrigal_amd import _lib
    syms = _lib.declared_symbols()
    L = _lib.lib()
    for s in NEW:
        assert s in syms and hasattr(L, s), s
    assert L.mdg_bilinear_bincount_max_edges() >= 1024
    assert L.mdg_abi_version() >= 14


def test_bincount_workspace_is_the_operand_images():
    from madrigal_amd import _lib
    L = _lib.lib()
    assert L.mdg_bilinear_bincount_workspace_bytes(4096, 4096, 896, 128, 1000, 0) == 0
    for prec in (1, 2, 3):
        assert (L.mdg_bilinear_bincount_workspace_bytes(4096, 4096, 896, 128, 1000, prec)
                == L.mdg_bilinear_allpairs_workspace_bytes(4096, 4096, 896, 128, prec))


def test_c_entry_point_refuses_before_it_touches_a_device():
    from madrigal_amd._lib import lib
    L = lib()
    mx = L.mdg_bilinear_bincount_max_edges()
    for n_tail, n_edges, eligible, what in ((4, mx + 1, 0, b"n_edges must be"), (4, 0, 0, b"n_edges must be"), (5, 3, 2, b"one drug set"),
                                            (5, 3, 1, b"one drug set"), (4, 3, 7, b"unknown eligible"), (1 << 23, 3, 0, b"2^23")):
        n_head = 4 if n_tail < 100 else n_tail
        rc = L.mdg_bilinear_bincount(None, None, None, None, None, n_head, n_tail, 1, 128, n_edges, 0, eligible, None, 0, None)
        assert rc == -1 and what in L.mdg_last_error(), (n_tail, n_edges, eligible, L.mdg_last_error())
    assert L.mdg_bilinear_bincount(None, None, None, None, None, 4, 4, 1, 64, 3, 0, 0, None, 0, None) == -1


def test_ranks_from_counts_reproduces_the_reference(golden):
    """tests/golden/ranks.npz holds the reference's own normalised ranks of [3,37,37] scores.  For every strict-lower-triangle
    entry whose score is unique in its outcome, ranks_from_counts(number of lower-triangle scores below it, 37) is that value,
    bit for bit."""
    from madrigal_amd.pipeline import ranks_from_counts
    g = golden("ranks")
    S, ref = torch.from_numpy(g["scores"]), torch.from_numpy(g["normalized"])
    N = S.shape[1]
    ii, jj = torch.tril_indices(N, N, -1)
    vals = S[:, ii, jj]
    less = brute_less(vals, vals)
    uniq = is_unique(vals, vals)
    assert float(uniq.float().mean()) > 0.9
    got = ranks_from_counts(less, N)
    assert got.dtype == torch.float32 and got.shape == vals.shape
    assert torch.equal(got[uniq], ref[:, ii, jj][uniq])
    assert torch.equal(ranks_from_counts(torch.tensor([0, N * (N - 1) // 2 - 1]), N), torch.tensor([1 / (N * (N - 1) / 2), 1.0]).float())


def test_wrapper_validation_without_a_gpu():
    from madrigal_amd import ops
    mx = ops.bilinear_bincount_max_edges()
    assert mx >= 1024
    z, z2, w = torch.zeros(6, 128), torch.zeros(4, 128), torch.zeros(2, 128, 128)
    up = torch.tensor([[0.0, 1.0, 1.0, 2.0]] * 2)
    bad = {
        "ascending": up.flip(1),
        "finite": torch.tensor([[0.0, float("nan"), 1.0]] * 2),
        "finite ": torch.tensor([[0.0, 1.0, float("inf")]] * 2),
        "edges per outcome": torch.zeros(2, 0),
        "edges per outcome ": torch.zeros(2, mx + 1),
        "one row per outcome": up[:1],
        "one row per outcome ": torch.cat([up, up[:1]]),
        "2 dims": up[0],
    }
    for what, e in bad.items():
        with pytest.raises(ValueError, match=what.strip()):
            ops.bilinear_bincount(z, z, w, e)
    with pytest.raises(ValueError, match="one drug set"):
        ops.bilinear_bincount(z, z2, w, up, eligible="lower")
    with pytest.raises(ValueError, match="one drug set"):
        ops.bilinear_bincount(z, z2, w, up, eligible="not_self")
    with pytest.raises(ValueError, match="unknown eligible"):
        ops.bilinear_bincount(z, z, w, up, eligible="upper")
    with pytest.raises(ValueError, match="unknown precision"):
        ops.bilinear_bincount(z, z, w, up, precision="fp8")
    with pytest.raises(ValueError, match="feature dims"):
        ops.bilinear_bincount(z[:, :64], z, w, up)
    with pytest.raises(ValueError, match="float32"):
        ops.bilinear_bincount(z, z, w, up.double())
    # a well-formed call on CPU tensors: the HIP path has no CPU fallback
    with pytest.raises(ValueError, match="GPU"):
        ops.bilinear_bincount(z, z, w, up)
    with pytest.raises(ValueError, match="GPU"):
        ops.bilinear_bincount(z, z2, w, up, eligible="all")
