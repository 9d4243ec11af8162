"""CPU checks of the split counting product: the C ABI declares and exports mdg_bilinear_bincount_split, and the two pure
functions built on its counts -- pipeline.recovery_from_counts and pipeline.auroc_bounds_from_counts -- equal brute force over a
dense score tensor and a dense symmetric known-pair mask (counts by torch.bucketize per class, AUROC by rank sum with ties 1/2)."""
import inspect
import math

import pytest
import torch

L, N = 3, 40


def test_the_split_entry_point_is_declared_and_exported():
    from madrigal_amd import _lib
    lib = _lib.lib()
    assert lib.mdg_abi_version() >= 20
    protos = _lib.declared_prototypes()
    name = "mdg_bilinear_bincount_split"
    assert name in _lib.declared_symbols() and name in protos and hasattr(lib, name)
    # the twin's arguments plus (mask, plane_stride)
    assert protos[name][1][:-2] == protos["mdg_bilinear_bincount"][1] and len(protos[name][1]) == len(protos["mdg_bilinear_bincount"][1]) + 2
    assert protos[name][1][-2:] == protos["mdg_bilinear_select_count_masked"][1][-2:]


def _dense_case(unique: bool):
    """Scores [L, N, N] (rounded to a coarse grid unless ``unique``: ties within and across the classes), a symmetric bool mask
    [N, N] with the diagonal also set, and the strict-lower-triangle values / class flags [L, M]."""
    g = torch.Generator().manual_seed(3 if unique else 4)
    dense = torch.randn((L, N, N), generator=g)
    if not unique:
        dense = (dense * 4).round() / 4
    known = torch.rand((N, N), generator=g) < 0.2
    known = known | known.T | torch.eye(N, dtype=torch.bool)
    ii, jj = torch.tril_indices(N, N, -1)
    vals = dense[:, ii, jj].contiguous()
    cls = known[ii, jj]
    assert vals.shape == (L, N * (N - 1) // 2) and 0 < int(cls.sum()) < cls.numel()
    if unique:
        assert all(int(torch.unique(vals[l]).numel()) == vals.shape[1] for l in range(L))
    return dense, known, vals, cls


def _split_counts(vals, cls, edges):
    """[2, L, B+1]: torch.bucketize(right=True) + bincount of each class."""
    B = edges.shape[1]
    out = torch.zeros((2, L, B + 1), dtype=torch.int64)
    for l in range(L):
        b = torch.bucketize(vals[l], edges[l].contiguous(), right=True)
        for p in (0, 1):
            out[p, l] = torch.bincount(b[cls == bool(p)], minlength=B + 1)
    return out


def _exact_auroc(v, pos):
    """Rank-sum AUROC with ties counted 1/2, in float64: P(score of a positive > score of a negative) + P(equal) / 2."""
    p, n = v[pos].double(), v[~pos].double()
    gt = (p[:, None] > n[None, :]).sum().item()
    eq = (p[:, None] == n[None, :]).sum().item()
    return (gt + 0.5 * eq) / (p.numel() * n.numel())


def test_recovery_from_counts_equals_brute_force():
    from madrigal_amd.pipeline import recovery_from_counts
    _, _, vals, cls = _dense_case(unique=False)
    g = torch.Generator().manual_seed(8)
    cuts = torch.cat([vals[:, torch.randperm(vals.shape[1], generator=g)[:9]], torch.randn((L, 4), generator=g)], 1)     # unsorted; some ARE scores
    cuts[:, 5] = cuts[:, 2]                                                                                                # a repeat
    less_all = (vals[:, None, :] < cuts[:, :, None]).sum(2)
    less_known = ((vals[:, None, :] < cuts[:, :, None]) & cls[None, None, :]).sum(2)
    total, n_known = vals.shape[1], int(cls.sum())
    got = recovery_from_counts(less_all, less_known, total, n_known)
    sel = (vals[:, None, :] >= cuts[:, :, None])
    selected = sel.sum(2)
    hits = (sel & cls[None, None, :]).sum(2)
    assert got["selected"].dtype == torch.int64 and got["hits"].dtype == torch.int64
    assert torch.equal(got["selected"], selected) and torch.equal(got["hits"], hits)
    assert bool((selected > 0).all())
    for key, ref in (("precision", hits.double() / selected.double()), ("recall", hits.double() / n_known),
                     ("enrichment", hits.double() / selected.double() / (n_known / total))):
        assert got[key].dtype == torch.float64 and got[key].shape == cuts.shape
        assert torch.allclose(got[key], ref, rtol=1e-14, atol=0), key
    # per-outcome class sizes as tensors broadcast like the ints
    again = recovery_from_counts(less_all, less_known, torch.full((L, 1), total), torch.full((L, 1), n_known))
    assert all(torch.equal(again[k], got[k]) for k in got)


def test_recovery_nan_cases():
    from madrigal_amd.pipeline import recovery_from_counts
    # cut above every score: nothing selected -> precision NaN, recall 0
    r = recovery_from_counts(torch.tensor([[780, 700]]), torch.tensor([[50, 45]]), 780, 50)
    assert r["selected"].tolist() == [[0, 80]] and r["hits"].tolist() == [[0, 5]]
    assert math.isnan(r["precision"][0, 0]) and math.isnan(r["enrichment"][0, 0]) and r["recall"][0, 0] == 0.0
    assert r["precision"][0, 1] == 5 / 80 and r["recall"][0, 1] == 0.1
    # nothing known: recall NaN, precision 0
    r = recovery_from_counts(torch.tensor([[700]]), torch.tensor([[0]]), 780, 0)
    assert math.isnan(r["recall"][0, 0]) and r["precision"][0, 0] == 0.0 and r["hits"][0, 0] == 0


@pytest.mark.parametrize("n_edges", [1, 7, 64])
def test_auroc_bounds_bracket_the_exact_value(n_edges):
    from madrigal_amd.pipeline import auroc_bounds_from_counts
    _, _, vals, cls = _dense_case(unique=False)
    edges = torch.linspace(-2.5, 2.5, n_edges)[None, :].expand(L, -1).contiguous() if n_edges > 1 else torch.zeros((L, 1))
    counts = _split_counts(vals, cls, edges)
    assert torch.equal(counts.sum((0, 2)), torch.full((L,), vals.shape[1]))
    lower, upper = auroc_bounds_from_counts(counts)
    assert lower.dtype == torch.float64 and upper.dtype == torch.float64 and lower.shape == (L,)
    for l in range(L):
        exact = _exact_auroc(vals[l], cls)
        assert 0.0 <= float(lower[l]) <= exact <= float(upper[l]) <= 1.0, (l, float(lower[l]), exact, float(upper[l]))
    # the formulas, written out with Python integers
    for l in range(L):
        u, k = counts[0, l].tolist(), counts[1, l].tolist()
        lo_i = sum(k[b] * sum(u[:b]) for b in range(len(u)))
        up_i = lo_i + sum(k[b] * u[b] for b in range(len(u)))
        assert float(lower[l]) == lo_i / (sum(k) * sum(u)) and float(upper[l]) == up_i / (sum(k) * sum(u))


def test_auroc_bounds_meet_with_an_edge_at_every_distinct_score():
    """780 unique scores per outcome < 1024 edges: every bin holds one pair, no known and novel pair share one, lower == upper ==
    the exact value."""
    from madrigal_amd.pipeline import auroc_bounds_from_counts
    _, _, vals, cls = _dense_case(unique=True)
    edges = torch.sort(vals, dim=1).values.contiguous()
    assert edges.shape[1] == 780
    lower, upper = auroc_bounds_from_counts(_split_counts(vals, cls, edges))
    assert torch.equal(lower, upper)
    for l in range(L):
        assert abs(float(lower[l]) - _exact_auroc(vals[l], cls)) <= 1e-15


def test_auroc_bounds_nan_without_a_class():
    from madrigal_amd.pipeline import auroc_bounds_from_counts
    counts = torch.tensor([[[3, 4, 5], [0, 0, 0], [1, 0, 2]], [[0, 0, 0], [2, 2, 2], [1, 1, 0]]])       # K = 0; U = 0; both present
    lower, upper = auroc_bounds_from_counts(counts)
    assert math.isnan(lower[0]) and math.isnan(upper[0]) and math.isnan(lower[1]) and math.isnan(upper[1])
    assert float(lower[2]) == (1 * 1) / (2 * 3) and float(upper[2]) == (1 * 1 + 1 * 1) / (2 * 3)
    with pytest.raises(ValueError):
        auroc_bounds_from_counts(counts[0])


def test_signatures_accept_known_none():
    from madrigal_amd import models, ops, pipeline
    for fn in (pipeline.score_histogram, pipeline.count_below):
        p = inspect.signature(fn).parameters["known"]
        assert p.default is None
    assert inspect.signature(ops.bilinear_bincount).parameters["split"].default is None
    assert inspect.signature(models.BilinearDDIScorer.bincount).parameters["split"].default is None
    for name in ("recovery_from_counts", "recovery_at_cuts", "auroc_bounds_from_counts", "auroc_bounds"):
        assert callable(getattr(pipeline, name))
