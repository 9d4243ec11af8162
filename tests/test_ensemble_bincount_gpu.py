"""Counting the checkpoint ensemble's probabilities between edges on the GPU (ops.bilinear_ensemble_bincount,
pipeline.ensemble_score_histogram / ensemble_count_below / ensemble_normalized_ranks_of / ensemble_recovery_at_cuts /
ensemble_auroc_bounds) against the dense ensemble product, exactly.

The reference is always the GENERAL ensemble sweep on the card, ``ops.bilinear_ensemble_sigmoid(zh, [t.clone() for t in zt], ws)`` (the
clone on the tail side forces the non-mirrored sweep; tests/test_ensemble_select_gpu.py's generator and cache, so a case the two files
share is computed once), then per outcome ``torch.bucketize(P[l][allowed], edges[l], right=True)`` and ``torch.bincount``; with
``split=`` the same per class of the dense mask.  Every comparison is ``torch.equal`` on integers: no tolerance is involved.

Two input regimes (z ~ N(0,1) * scale): scale 0.3, no probability is 0 or 1; scale 1.0, a real tie set at exactly 1.0 (K = 1, 2)."""
import functools

import pytest
import torch

from test_ensemble_select_gpu import L, _allowed, _case, _random_pairs, _shape

pytestmark = pytest.mark.gpu


def _attained_at(plane, qs):
    """The values of ``plane`` at its dense quantiles ``qs``, ascending: attained values, so ``<=`` is tested on equality, and equal
    neighbours among them (ties, or more edges than values) are edges between equal values."""
    flat = torch.sort(plane.reshape(-1)).values
    idx = (torch.as_tensor(qs, dtype=torch.float64) * (flat.numel() - 1)).long().to(flat.device)
    return flat[idx]


def _edge_sets(P):
    """name -> fp32 [L, B] on the card; a different row per outcome, each aimed at a branch of the epilogue."""
    from madrigal_amd import ops
    dev = P.device
    t = lambda *rows: torch.stack([torch.as_tensor(r, dtype=torch.float32, device=dev) for r in rows]).contiguous()   # noqa: E731
    big = ops.bilinear_bincount_max_edges()
    lin = lambda a, b, n: torch.linspace(a, b, n, device=dev)     # noqa: E731
    top = torch.sort(P[2].reshape(-1)).values[-big:]              # the strongest values of outcome 2: the fast-path regime
    top = torch.cat([top[:1].repeat(big - top.numel()), top])
    return {
        "B1": t(_attained_at(P[0], [0.99]), [0.5], [1.0]),
        # every value inside the bracket: the slow path alone; both edges below 0 / above 1: the fast path alone
        "B2": t([-1.0, 2.0], [-2.0, -1.0], [1.5, 2.0]),
        # 0.0 and 1.0 as edges; equal neighbouring edges at an attained value (an empty bin); 1.0 then 1.5 (the bin after the ties is empty)
        "B3": t(torch.cat([torch.zeros(1, device=dev), _attained_at(P[0], [0.5]), torch.ones(1, device=dev)]),
                _attained_at(P[1], [0.25, 0.25, 0.75]), [0.5, 1.0, 1.5]),
        "B5": t(_attained_at(P[0], [0.1, 0.3, 0.5, 0.7, 0.9]), [-1.0, 0.0, 0.5, 1.0, 2.0], lin(0.45, 0.55, 5)),
        "B1000": t(_attained_at(P[0], torch.linspace(0, 1, 1000).tolist()), lin(0.0, 1.0, 1000), lin(0.4, 0.6, 1000)),
        "Bmax": t(_attained_at(P[0], torch.linspace(0.5, 1, big).tolist()), lin(-1.0, 2.0, big), top),
    }


def _dense_counts(P, edges, eligible, cls=None):
    """int64 [L, B+1] of the dense P; ``cls``: bool [1 or L, nh, nt], only those pairs."""
    nl, nh, nt = P.shape
    ok = _allowed(nh, nt, eligible, P.device)
    out = []
    for l in range(nl):
        m = ok if cls is None else ok & cls[l if cls.shape[0] > 1 else 0]
        b = torch.bucketize(P[l][m].contiguous(), edges[l].contiguous(), right=True)
        out.append(torch.bincount(b, minlength=edges.shape[1] + 1))
    return torch.stack(out)


def _n_eligible(nh, nt, eligible):
    return {"all": nh * nt, "not_self": nh * (nh - 1), "lower": nh * (nh - 1) // 2}[eligible]


def _check(zh, zt, ws, P, eligible, prec, what=()):
    from madrigal_amd import ops
    nh, nt = P.shape[1:]
    got = {}
    for name, edges in _edge_sets(P).items():
        c = ops.bilinear_ensemble_bincount(zh, zt, ws, edges, eligible=eligible, precision=prec)
        want = _dense_counts(P, edges, eligible)
        assert c.dtype == torch.int64 and c.shape == (L, edges.shape[1] + 1), what + (name,)
        assert torch.equal(c, want), what + (name, int((c != want).sum()))
        assert c.sum(1).tolist() == [_n_eligible(nh, nt, eligible)] * L, what + (name,)
        got[name] = c
    return got


# ---- sizes and edge sets -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("scale", [0.3, 1.0])
@pytest.mark.parametrize("K", [1, 2, 5, 8])
@pytest.mark.parametrize("shape", ["1x1", "33x65", "129x130", "chunk-1", "chunk", "chunk+1", "300x1001"])
def test_sizes_and_edge_sets_against_the_dense_product(shape, K, scale, prec):
    nh, nt = _shape(shape)
    zh, zt, ws, P = _case(K, nh, nt, scale, prec, False)
    c = _check(zh, zt, ws, P, "all", prec)
    n = nh * nt
    assert c["B2"].tolist() == [[0, n, 0], [0, 0, n], [n, 0, 0]]          # all inside; all above both edges; all below both
    ones = int((P[2] == 1.0).sum())
    assert c["B3"][2].tolist()[2:] == [ones, 0] and int(c["B1"][2, 1]) == ones   # the tie set at 1.0 sits in [1.0, 1.5); nothing above
    assert int(c["B3"][0, 0]) == 0 and int(c["B3"][1, 1]) == 0          # nothing below 0.0; equal neighbouring edges: an empty bin
    if scale == 1.0 and K <= 2 and n > 100000:
        assert ones > 0
    if scale == 0.3:
        assert ones == 0


@pytest.mark.parametrize("K,scale", [(5, 0.3), (1, 1.0)])
def test_two_launches_agree_bit_for_bit(K, scale):
    from madrigal_amd import ops
    zh, zt, ws, P = _case(K, 300, 1001, scale, "bf16x3", False)
    h, t = torch.arange(0, 300, 3), torch.arange(0, 1000, 10)
    mask = ops.pair_mask(h, t, 300, 1001, device="cuda")
    for name, edges in _edge_sets(P).items():
        a = ops.bilinear_ensemble_bincount(zh, zt, ws, edges)
        b = ops.bilinear_ensemble_bincount(zh, zt, ws, edges)
        assert torch.equal(a, b), name
        a = ops.bilinear_ensemble_bincount(zh, zt, ws, edges, split=mask)
        b = ops.bilinear_ensemble_bincount(zh, zt, ws, edges, split=mask)
        assert torch.equal(a, b), name


# ---- eligibility ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("K,scale", [(5, 0.3), (1, 1.0), (2, 1.0)])
@pytest.mark.parametrize("eligible", ["not_self", "lower"])
@pytest.mark.parametrize("N", [1, 2, 33, 129, 300, 513])
def test_one_drug_set_against_itself(N, eligible, K, scale, prec):
    """129, 300 and 513 end in a partial row block (rows >= n_head and columns >= n_tail add nothing: every row of the result sums
    to the number of eligible pairs); 300 and 513 have several row blocks, and LOWER skips the tiles above the diagonal."""
    z, _, ws, P = _case(K, N, N, scale, prec, True)
    _check(z, z, ws, P, eligible, prec)


# ---- split ---------------------------------------------------------------------------------------------------------------------
def _check_split(zh, zt, ws, P, mask, eligible, prec, sets=("B1", "B2", "B3", "B5", "B1000", "Bmax"), what=()):
    """Both tables against the dense per-class counts, and their sum against the unsplit call."""
    from madrigal_amd import ops
    nh, nt = P.shape[1:]
    known = ops.pair_mask_dense(mask, nh, nt)
    all_edges = _edge_sets(P)
    out = {}
    for name in sets:
        edges = all_edges[name]
        c = ops.bilinear_ensemble_bincount(zh, zt, ws, edges, eligible=eligible, precision=prec, split=mask)
        assert c.dtype == torch.int64 and c.shape == (2, L, edges.shape[1] + 1), what + (name,)
        assert torch.equal(c[0], _dense_counts(P, edges, eligible, ~known)), what + (name, "novel")
        assert torch.equal(c[1], _dense_counts(P, edges, eligible, known)), what + (name, "known")
        assert torch.equal(c.sum(0), ops.bilinear_ensemble_bincount(zh, zt, ws, edges, eligible=eligible, precision=prec)), what + (name,)
        out[name] = c
    return out


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("K,scale", [(5, 0.3), (1, 1.0)])
@pytest.mark.parametrize("planes", ["shared", "per_outcome"])
@pytest.mark.parametrize("eligible", ["not_self", "lower"])
def test_split_by_a_random_mask_with_a_full_row(eligible, planes, K, scale, prec):
    """1 % of the pairs at random plus every bit of row 7, symmetric: the mask has bits on the diagonal and above it, which change
    nothing under not_self / lower (an ineligible pair is in neither table)."""
    from madrigal_amd import ops
    N = 300
    z, _, ws, P = _case(K, N, N, scale, prec, True)
    h, t = _random_pairs(N, 0.01, 5)
    h = torch.cat([h, torch.full((N,), 7), torch.arange(N)])                 # ... and the whole diagonal
    t = torch.cat([t, torch.arange(N), torch.arange(N)])
    if planes == "shared":
        mask = ops.pair_mask(h, t, N, symmetric=True, device="cuda")
    else:
        mask = ops.pair_mask(h, t, N, labels=torch.arange(h.numel()) % L, n_labels=L, symmetric=True, device="cuda")
    c = _check_split(z, z, ws, P, mask, eligible, prec)
    n_known = (ops.pair_mask_dense(mask, N, N) & _allowed(N, N, eligible)[None]).sum((1, 2))       # the diagonal and the upper triangle count for nothing
    assert c["B1"][1].sum(1).tolist() == n_known.expand(L).tolist()


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("eligible", ["all", "lower"])
def test_split_by_an_empty_mask_and_by_a_bit_in_every_tile(eligible, prec):
    from madrigal_amd import ops
    chunk = 64 * ops.bilinear_ensemble_topk_chunk_tiles()
    nh, nt = (129, chunk + 1) if eligible == "all" else (513, 513)
    zh, zt, ws, P = _case(2, nh, nt, 1.0, prec, eligible != "all")
    zt = zt if eligible == "all" else zh
    for planes in (1, L):
        zero = torch.zeros((planes, (nh + 31) // 32, (nt + 63) // 64 * 64), dtype=torch.int32, device="cuda")
        c = _check_split(zh, zt, ws, P, zero, eligible, prec)
        assert all(not bool(v[1].any()) for v in c.values())
    # one bit per (row block of 32, column tile of 64), at a place that moves with both; the last, partial ones included
    rb, ct = torch.arange((nh + 31) // 32), torch.arange((nt + 63) // 64)
    h = (32 * rb[:, None] + (5 * rb[:, None] + 3 * ct[None, :]) % 32).reshape(-1)
    t = (64 * ct[None, :] + (7 * rb[:, None] + 11 * ct[None, :]) % 64).reshape(-1)
    keep = (h < nh) & (t < nt)
    every = ops.pair_mask(h[keep], t[keep], nh, nt, device="cuda")
    _check_split(zh, zt, ws, P, every, eligible, prec)
    # every bit set: table 0 is empty
    full = torch.full_like(every, -1)
    c = _check_split(zh, zt, ws, P, full, eligible, prec, sets=("B3", "B1000"))
    assert all(not bool(v[0].any()) for v in c.values())


@pytest.mark.parametrize("eligible", ["not_self", "lower"])
def test_split_by_the_pairs_at_or_above_an_attained_cut(eligible):
    """The mask holds, outcome by outcome, exactly the eligible pairs with P >= an attained value: with that value as the one edge,
    table 1 is all in the upper bin and table 0 all in the lower."""
    from madrigal_amd import ops
    N = 300
    z, _, ws, P = _case(5, N, N, 0.3, "bf16x3", True)
    cut = torch.stack([_attained_at(P[l], [0.99])[0] for l in range(L)])
    idx = torch.nonzero((P >= cut[:, None, None]) & _allowed(N, N, eligible)[None])
    mask = ops.pair_mask(idx[:, 1], idx[:, 2], N, labels=idx[:, 0], n_labels=L, device="cuda")
    c = _check_split(z, z, ws, P, mask, eligible, "bf16x3", sets=("B1", "B5"))
    got = ops.bilinear_ensemble_bincount(z, z, ws, cut[:, None].contiguous(), eligible=eligible, split=mask)
    n_hits = torch.bincount(idx[:, 0], minlength=L)
    assert torch.equal(got[1], torch.stack([torch.zeros_like(n_hits), n_hits], 1))
    assert torch.equal(got[0], torch.stack([_n_eligible(N, N, eligible) - n_hits, torch.zeros_like(n_hits)], 1))
    assert int(n_hits.min()) > 0 and c["B1"].shape == (2, L, 2)


# ---- the sibling products: the same sweep, the same bits ---------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("K,scale", [(5, 0.3), (1, 1.0)])
@pytest.mark.parametrize("eligible", ["all", "not_self", "lower"])
def test_one_edge_agrees_with_select_count(eligible, K, scale, prec):
    from madrigal_amd import ops
    N = 300
    same = eligible != "all"
    zh, zt, ws, P = _case(K, N, N if same else 1001, scale, prec, same)
    nt = P.shape[2]
    thr = torch.stack([_attained_at(P[0], [0.99])[0], torch.tensor(0.5, device="cuda"), torch.tensor(1.0, device="cuda")])
    c = ops.bilinear_ensemble_bincount(zh, zt, ws, thr[:, None].contiguous(), eligible=eligible, precision=prec)
    sel = ops.bilinear_ensemble_select_count(zh, zt, ws, thr, eligible=eligible, precision=prec)
    assert torch.equal(c[:, 1], sel.sum(1, dtype=torch.int64))
    h, t = torch.randint(0, N, (900,), generator=torch.Generator().manual_seed(3)), torch.randint(0, nt, (900,), generator=torch.Generator().manual_seed(4))
    mask = ops.pair_mask(h, t, N, nt, device="cuda")
    cs = ops.bilinear_ensemble_bincount(zh, zt, ws, thr[:, None].contiguous(), eligible=eligible, precision=prec, split=mask)
    selx = ops.bilinear_ensemble_select_count(zh, zt, ws, thr, eligible=eligible, precision=prec, exclude=mask)
    assert torch.equal(cs[0, :, 1], selx.sum(1, dtype=torch.int64))
    assert torch.equal(cs.sum(0), c)


def test_empty_sizes_and_device_refusals():
    from madrigal_amd import ops
    z = [torch.randn(6, 128, device="cuda") for _ in range(2)]
    w = [torch.randn(2, 128, 128, device="cuda") for _ in range(2)]
    e = torch.tensor([[0.25, 0.5, 0.75]] * 2, device="cuda")
    assert ops.bilinear_ensemble_bincount(z, z, [t[:0] for t in w], e[:0]).shape == (0, 4)
    c = ops.bilinear_ensemble_bincount([t[:0] for t in z], z, w, e)
    assert c.shape == (2, 4) and c.dtype == torch.int64 and not bool(c.any())
    c = ops.bilinear_ensemble_bincount(z, [t[:0] for t in z], w, e)
    assert c.shape == (2, 4) and not bool(c.any())
    zero = torch.zeros((1, 1, 64), dtype=torch.int32, device="cuda")
    c = ops.bilinear_ensemble_bincount(z, z, w, e, eligible="lower", split=zero)
    assert c.shape == (2, 2, 4) and c[0].sum(1).tolist() == [15, 15] and not bool(c[1].any())
    with pytest.raises(ValueError, match="GPU"):
        ops.bilinear_ensemble_bincount(z, z, w, e.cpu())
    with pytest.raises(ValueError, match="ascending"):
        ops.bilinear_ensemble_bincount(z, z, w, e.flip(1))
    with pytest.raises(ValueError, match="planes"):
        ops.bilinear_ensemble_bincount(z, z, w, e, split=torch.zeros((3, 1, 64), dtype=torch.int32, device="cuda"))


# ---- pipeline ---------------------------------------------------------------------------------------------------------------------
N_DRUGS, N_OUT = 130, 6


@functools.lru_cache(maxsize=None)
def _checkpoints():
    """Three configs.build_model checkpoints (drugbank163 layout, 6 outcomes) differing by seed, and the embeddings of 130 drugs from
    generate_embeddings under each."""
    from madrigal_amd import configs, data as D, models as M
    from madrigal_amd.pipeline import generate_embeddings
    n = N_DRUGS
    batch, bkg = D.make_batch(n, 5, kg_nodes=900, kg_edges=6000)
    b = D.batch_to(batch, "cuda")
    kgc = {"data": bkg["data"].to("cuda"), "drug_index_map": bkg["drug_index_map"].cuda()}
    filler = torch.randn((n, 128), generator=torch.Generator().manual_seed(6)).cuda()
    models, zs = [], []
    for seed in (3, 4, 5):
        torch.manual_seed(seed)
        model = configs.build_model("drugbank163", bkg["data"], N_OUT).cuda().eval()
        with M.precision("bf16x3"):
            z = generate_embeddings(model, b, kgc, kg_filler=filler).contiguous()
        assert z.shape == (n, 128) and bool(torch.isfinite(z).all())
        models.append(model)
        zs.append(z)
    return models, zs


@functools.lru_cache(maxsize=None)
def _pipeline_case(prec):
    """(models, zs, dense P [6, N, N] of the general sweep, its strict lower triangle [6, M], a shared and a per-outcome known mask)."""
    from madrigal_amd import models as M
    from madrigal_amd.pipeline import ensemble_all_pairs, known_pairs_mask
    models, zs = _checkpoints()
    with M.precision(prec), torch.no_grad():
        dense = ensemble_all_pairs(models, zs, drug_2_inds=list(range(N_DRUGS))).contiguous()   # an index list on the tail side: the general sweep
    low = dense[:, _allowed(N_DRUGS, N_DRUGS, "lower")]
    g = torch.Generator().manual_seed(12)
    kh, kt = torch.randint(0, N_DRUGS, (400,), generator=g), torch.randint(0, N_DRUGS, (400,), generator=g)
    shared = known_pairs_mask(N_DRUGS, kh, kt, device="cuda")
    per = known_pairs_mask(N_DRUGS, kh, kt, labels=torch.arange(400) % (N_OUT - 1), n_labels=N_OUT, device="cuda")   # the last outcome has no known pair
    return models, zs, dense, low, shared, per


def _less(low, q):
    """int64 [L', Q]: the entries of low [L', M] strictly below every query."""
    return (low[:, None, :] < q[:, :, None]).sum(2)


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_ranks_of_the_top_pairs_and_counts_below_many_queries(prec):
    from madrigal_amd import models as M, ops
    from madrigal_amd.pipeline import ensemble_count_below, ensemble_normalized_ranks_of, ensemble_top_pairs, ranks_from_counts
    models, zs, dense, low, shared, per = _pipeline_case(prec)
    with M.precision(prec):
        tv = ensemble_top_pairs(models, zs, 50)[0]
        ranks = ensemble_normalized_ranks_of(models, zs, tv)
        assert ranks.dtype == torch.float32 and ranks.shape == (N_OUT, 50)
        assert torch.equal(ranks, ranks_from_counts(_less(low, tv), N_DRUGS))
        assert bool((ranks[:, :-1] >= ranks[:, 1:]).all()) and float(ranks.max()) <= 1.0
        # Q = 2100 unsorted queries with repeats: more than 2048 distinct values per outcome, three sweeps
        g = torch.Generator().manual_seed(7)
        q = torch.rand((N_OUT, 2100), generator=g).cuda()
        pick = torch.randint(0, low.shape[1], (N_OUT, 30), generator=g).cuda()
        q[:, 2060:2090] = torch.gather(low, 1, pick)                # attained values
        q[:, 2090:] = q[:, 5:15]                                    # repeats
        q = q[:, torch.randperm(2100, generator=g).cuda()].contiguous()
        assert min(int(torch.unique(r).numel()) for r in q) > 2 * ops.bilinear_bincount_max_edges()
        got = ensemble_count_below(models, zs, q)
        assert got.dtype == torch.int64 and torch.equal(got, _less(low, q))
        # split by the known network, and an outcome sub-range
        known = ops.pair_mask_dense(per, N_DRUGS, N_DRUGS)[:, _allowed(N_DRUGS, N_DRUGS, "lower")]      # [6, M]
        both = ensemble_count_below(models, zs, q[:, :70], known=per)
        below = low[:, None, :] < q[:, :70, None]
        assert torch.equal(both[1], (below & known[:, None, :]).sum(2)) and torch.equal(both[0], (below & ~known[:, None, :]).sum(2))
        assert torch.equal(ensemble_count_below(models, zs, q[2:5], label_range=(2, 5)), got[2:5])
        assert torch.equal(ensemble_count_below(models, zs, q[2:5, :70], label_range=(2, 5), known=per), both[:, 2:5])
        assert torch.equal(ensemble_normalized_ranks_of(models, zs, tv[1:3], label_range=(1, 3)), ranks[1:3])
        assert ensemble_count_below(models, zs, q[:, :0]).shape == (N_OUT, 0)


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_histograms_recovery_and_auroc_bounds(prec):
    from madrigal_amd import models as M, ops
    from madrigal_amd.pipeline import (auroc_bounds_from_counts, ensemble_auroc_bounds, ensemble_recovery_at_cuts, ensemble_score_histogram,
                                       ensemble_top_pairs)
    models, zs, dense, low, shared, per = _pipeline_case(prec)
    N = N_DRUGS
    with M.precision(prec):
        one = torch.linspace(0.0, 1.0, 41, device="cuda")
        rows = torch.stack([torch.sort(low[l]).values[torch.linspace(0, low.shape[1] - 1, 200).long()] for l in range(N_OUT)]).contiguous()
        for edges in (one, rows):
            e2 = edges if edges.dim() == 2 else edges[None].expand(N_OUT, -1)
            for eligible in ("lower", "not_self", "all"):
                h = ensemble_score_histogram(models, zs, edges, eligible=eligible)
                assert h.dtype == torch.int64 and torch.equal(h, _dense_counts(dense, e2, eligible))
            assert torch.equal(ensemble_score_histogram(models, zs, edges[..., :7] if edges.dim() == 1 else edges[1:4], label_range=(1, 4)),
                               _dense_counts(dense[1:4], (e2[:, :7] if edges.dim() == 1 else e2)[1:4], "lower"))
            for mask in (shared, per):
                cls = ops.pair_mask_dense(mask, N, N)
                hs = ensemble_score_histogram(models, zs, edges, known=mask)
                want = torch.stack([_dense_counts(dense, e2, "lower", ~cls), _dense_counts(dense, e2, "lower", cls)])
                assert hs.shape == (2, N_OUT, e2.shape[1] + 1) and torch.equal(hs, want)
                assert torch.equal(hs.sum(0), ensemble_score_histogram(models, zs, edges))
                lo_b, up_b = ensemble_auroc_bounds(models, zs, mask, edges)
                lo_w, up_w = auroc_bounds_from_counts(want)
                assert torch.equal(lo_b.isnan(), lo_w.isnan()) and torch.equal(lo_b.nan_to_num(-1), lo_w.nan_to_num(-1))
                assert torch.equal(up_b.nan_to_num(-1), up_w.nan_to_num(-1))
                part = ensemble_auroc_bounds(models, zs, mask, e2[2:5].contiguous(), label_range=(2, 5))
                assert torch.equal(part[0].nan_to_num(-1), lo_b[2:5].nan_to_num(-1)) and torch.equal(part[1].nan_to_num(-1), up_b[2:5].nan_to_num(-1))
                # the exact tie-aware AUROC over the dense lower triangle lies inside, for every outcome with both classes
                kl = cls[:, _allowed(N, N, "lower")].expand(N_OUT, -1)
                for l in range(N_OUT):
                    pos, neg = low[l][kl[l]], low[l][~kl[l]]
                    if pos.numel() == 0 or neg.numel() == 0:
                        assert bool(lo_b[l].isnan()) and bool(up_b[l].isnan())
                        continue
                    gt = (pos[:, None] > neg[None, :]).sum().double()
                    eq = (pos[:, None] == neg[None, :]).sum().double()
                    auc = float((gt + 0.5 * eq) / (pos.numel() * neg.numel()))
                    assert float(lo_b[l]) - 1e-12 <= auc <= float(up_b[l]) + 1e-12, (l, float(lo_b[l]), auc, float(up_b[l]))
        assert bool(ensemble_auroc_bounds(models, zs, per, one)[0][N_OUT - 1].isnan())               # no known pair under the last outcome
        # recovery at cuts from the screen itself, unsorted, with a repeat
        tv = ensemble_top_pairs(models, zs, 20)[0]
        cuts = torch.cat([tv[:, [19, 0, 9, 9]], torch.full((N_OUT, 1), 0.5, device="cuda")], 1).contiguous()
        for mask in (shared, per):
            kl = ops.pair_mask_dense(mask, N, N)[:, _allowed(N, N, "lower")].expand(N_OUT, -1)
            r = ensemble_recovery_at_cuts(models, zs, mask, cuts)
            at = low[:, None, :] >= cuts[:, :, None]
            selected, hits = at.sum(2), (at & kl[:, None, :]).sum(2)
            assert torch.equal(r["selected"], selected) and torch.equal(r["hits"], hits)
            assert bool((r["selected"][:, 0] >= 20).all()) and bool((r["selected"][:, 1] >= 1).all())
            n_known = kl.sum(1, keepdim=True).double()
            prec_w = hits.double() / selected.double()
            assert torch.equal(r["precision"].nan_to_num(-1), prec_w.nan_to_num(-1))
            assert torch.equal(r["recall"].nan_to_num(-1), torch.where(n_known == 0, torch.full_like(prec_w, -1), hits.double() / n_known))
            sub = ensemble_recovery_at_cuts(models, zs, mask, cuts[3:6], label_range=(3, 6))
            assert torch.equal(sub["selected"], selected[3:6]) and torch.equal(sub["hits"], hits[3:6])
