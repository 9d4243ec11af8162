"""The split counting product on the GPU: mdg_bilinear_bincount_split against torch.bucketize + bincount of the project's own
dense head per class of the known-pair bitmap (exactly, in the fp32-grade modes), against the unsplit sweep (exactly, in all four
precisions), and the pipeline products built on it (count_below / score_histogram with ``known=``, recovery_at_cuts, auroc_bounds)
against the same quantities read off the dense score tensor."""
import pytest
import torch

from bincount_ref import brute_less, eligible_mask, eligible_scores, inputs

pytestmark = pytest.mark.gpu

L = 3
ALL_ONLY = [(33, 4), (300, 333)]
SQUARE = [(300, 300), (513, 513)]          # past a 256-row and a 512-row workgroup, ending on a ragged 64-column tile
MASKS = ["empty", "single", "random", "symmetric", "rows", "full"]


@pytest.fixture(scope="module")
def ops():
    from madrigal_amd import ops as _ops
    return _ops


def _modes(nh, nt):
    return ["all", "not_self", "lower"] if (nh, nt) in SQUARE else ["all"]


def _edge_sets(dense, eligible, max_edges):
    """The edge sets of test_bincount_gpu: one edge at 0; 37 edges that ARE eligible scores of the outcome, one of them twice;
    max_edges edges past both extremes; all edges below the minimum; all above the maximum (each fast path alone)."""
    vals = eligible_scores(dense, eligible)
    n_out, M = vals.shape
    lo, hi = float(vals.min()), float(vals.max())
    pick = torch.randint(0, M, (n_out, 37), generator=torch.Generator().manual_seed(7)).to(vals.device)
    real = torch.sort(torch.gather(vals, 1, pick), dim=1).values
    real[:, 11] = real[:, 10]
    line = lambda a, b, n: torch.linspace(a, b, n, device=vals.device)[None, :].expand(n_out, -1).contiguous()   # noqa: E731
    return {"zero": torch.zeros((n_out, 1), device=vals.device), "real": real.contiguous(), "wide": line(lo - 1, hi + 1, max_edges),
            "below": line(lo - 3, lo - 1, 5), "above": line(hi + 1, hi + 3, 5)}


def _pattern(name, nh, nt, P):
    """bool [P, nh, nt]: the listed pairs of every plane; with P > 1 the planes differ, so a wrong plane stride shows."""
    g = torch.Generator().manual_seed(17)
    m = torch.zeros((P, nh, nt), dtype=torch.bool)
    for p in range(P):
        if name == "single":
            m[p, min(nh - 1, 40 + p), min(nt - 1, 3)] = True
        elif name == "random":
            m[p] = torch.rand((nh, nt), generator=g) < 0.3
        elif name == "symmetric":                           # symmetric where the shape allows it, the diagonal also listed
            r = torch.rand((nh, nt), generator=g) < 0.05
            if nh == nt:
                r = r | r.T
            d = torch.arange(min(nh, nt))
            r[d, d] = True
            m[p] = r
        elif name == "rows":                                # whole words of ones next to whole words of zeros
            r0 = 32 + 32 * (p % 2) if nh > 96 else 32
            m[p, r0:r0 + 32] = True
        elif name == "full":
            m[p] = p != 1
    return m


def _mask_of(ops, name, nh, nt, P):
    """The pattern through ops.pair_mask: one shared plane (P = 1) or one plane per outcome (P = L)."""
    pl, h, t = torch.nonzero(_pattern(name, nh, nt, P), as_tuple=True)
    if P == 1:
        mask = ops.pair_mask(h, t, nh, nt)
    else:
        mask = ops.pair_mask(h, t, nh, nt, labels=pl, n_labels=P)
    assert mask.shape[0] == P
    return mask


def _class_flags(ops, mask, nh, nt, eligible):
    """bool [L, M]: the bit of every eligible entry (row-major, as eligible_scores lists them), from ops.pair_mask_dense."""
    dm = ops.pair_mask_dense(mask, nh, nt)
    flags = dm[:, eligible_mask(nh, nt, eligible, dm.device)]
    return flags.expand(L, -1) if flags.shape[0] == 1 else flags


def _split_ref(bins, flags, B):
    """int64 [2, L, B+1] from the bucket index of every eligible entry [L, M] and its class flag [L, M]."""
    out = torch.zeros((2, L, B + 1), dtype=torch.int64, device=bins.device)
    for l in range(L):
        both = torch.bincount(bins[l] + (B + 1) * flags[l].long(), minlength=2 * (B + 1))
        out[0, l], out[1, l] = both[:B + 1], both[B + 1:]
    return out


@pytest.mark.parametrize("nh,nt", ALL_ONLY + SQUARE)
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_split_counts_equal_bucketize_of_the_dense_general_sweep_per_class(ops, prec, nh, nt):
    """split[p] == torch.bucketize(right=True) + bincount of the eligible entries of the dense general sweep whose bit equals p;
    split.sum(0) == the unsplit call; a second launch gives the same."""
    zh, zt, w = inputs(nh, nt, L)
    zh, zt, ws = zh.cuda(), zt.cuda(), ops.symmetrize(w.cuda())
    dense = ops.bilinear_allpairs(zh, zt, ws, precision=prec)
    masks = {(name, P): _mask_of(ops, name, nh, nt, P) for name in MASKS for P in (1, L)}
    for eligible in _modes(nh, nt):
        vals = eligible_scores(dense, eligible)
        flags = {key: _class_flags(ops, m, nh, nt, eligible) for key, m in masks.items()}
        for ename, e in _edge_sets(dense, eligible, ops.bilinear_bincount_max_edges()).items():
            B = e.shape[1]
            bins = torch.stack([torch.bucketize(vals[l].contiguous(), e[l].contiguous(), right=True) for l in range(L)])
            twin = ops.bilinear_bincount(zh, zt, ws, e, eligible=eligible, precision=prec)
            for key, m in masks.items():
                got = ops.bilinear_bincount(zh, zt, ws, e, eligible=eligible, precision=prec, split=m)
                assert got.shape == (2, L, B + 1) and got.dtype == torch.int64
                ref = _split_ref(bins, flags[key], B)
                what = (eligible, ename, key, (got - ref).abs().sum().item())
                assert torch.equal(got, ref), what
                assert torch.equal(got.sum(0), twin), what
                if key[0] == "empty":
                    assert bool((got[1] == 0).all())
                if ename == "real":
                    assert torch.equal(ops.bilinear_bincount(zh, zt, ws, e, eligible=eligible, precision=prec, split=m), got), what


@pytest.mark.parametrize("nh,nt", SQUARE)
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_split_counts_of_the_16bit_sweeps(ops, prec, nh, nt):
    """The single-product modes (16x16x32, <= 2e-6 of the scale off the dense sweep): split.sum(0) == the unsplit call exactly (the
    same sweep: a disturbed vmcnt chain or a stale mask slot shows here); per table the cumulative counts lie between the dense
    class counts below e - delta and below e + delta, delta = 2e-6 max|dense|; each table's total is the class size exactly."""
    zh, zt, w = inputs(nh, nt, L)
    zh, zt, ws = zh.cuda(), zt.cuda(), ops.symmetrize(w.cuda())
    dense = ops.bilinear_allpairs(zh, zt, ws, precision=prec)
    delta = 2e-6 * float(dense.abs().max())
    masks = {(name, P): _mask_of(ops, name, nh, nt, P) for name in MASKS for P in (1, L)}
    for eligible in _modes(nh, nt):
        vals = eligible_scores(dense, eligible)
        sets = _edge_sets(dense, eligible, ops.bilinear_bincount_max_edges())
        twins = {ename: ops.bilinear_bincount(zh, zt, ws, e, eligible=eligible, precision=prec) for ename, e in sets.items()}
        for key, m in masks.items():
            flags = _class_flags(ops, m, nh, nt, eligible)
            # the dense values of every (class, outcome), sorted once (what brute_less sorts) and shared by the edge sets
            cls = [[torch.sort(vals[l][flags[l] == bool(p)].double()).values for l in range(L)] for p in (0, 1)]
            for ename, e in sets.items():
                got = ops.bilinear_bincount(zh, zt, ws, e, eligible=eligible, precision=prec, split=m)
                what = (eligible, ename, key)
                assert torch.equal(got.sum(0), twins[ename]), what
                C = torch.cumsum(got, 2)[:, :, :-1]
                for l in range(L):
                    for p in (0, 1):
                        assert int(got[p, l].sum()) == cls[p][l].numel(), what + (l, p)
                        lo = torch.searchsorted(cls[p][l], e[l].double() - delta, right=False)
                        hi = torch.searchsorted(cls[p][l], e[l].double() + delta, right=False)
                        assert bool((lo <= C[p, l]).all()) and bool((C[p, l] <= hi).all()), what + (l, p)


def test_c_level_refusals_launch_nothing_and_a_null_mask_is_the_twin(ops):
    from madrigal_amd._lib import lib
    n, B = 70, 3
    z = torch.randn(n, 128, device="cuda")
    w = ops.symmetrize(torch.randn(2, 128, 128, device="cuda"))
    e = torch.tensor([[-1.0, 0.0, 1.0]] * 2, device="cuda")
    per = ops.pair_mask([1, 5], [2, 3], n, n, labels=[0, 1], n_labels=2)
    counts = torch.full((2, 2, B + 1), -7, dtype=torch.int64, device="cuda")
    head = (z.data_ptr(), z.data_ptr(), w.data_ptr(), e.data_ptr(), counts.data_ptr(), n, n, 2, 128, B, 0)
    fn = lib().mdg_bilinear_bincount_split
    words = lib().mdg_pair_mask_plane_words(n, n)
    refused = [(head + (0, None, 0, None, per.data_ptr(), 5), b"plane_stride"),                   # neither 0 nor a whole plane
               (head + (0, None, 0, None, per.data_ptr(), words - 1), b"plane_stride"),
               (head + (0, None, 0, None, per.data_ptr() + 2, words), b"aligned"),                # a misaligned mask
               (head + (9, None, 0, None, per.data_ptr(), words), b"eligible"),                   # the twin's refusals
               (head[:9] + (lib().mdg_bilinear_bincount_max_edges() + 1, 0, 0, None, 0, None, per.data_ptr(), words), b"n_edges"),
               (head[:10] + (1, 0, None, 0, None, per.data_ptr(), words), b"workspace")]          # bf16x3 without its operand images
    for args, word in refused:
        assert fn(*args) != 0
        assert b"mdg_bilinear_bincount_split" in lib().mdg_last_error() and word in lib().mdg_last_error(), lib().mdg_last_error()
    torch.cuda.synchronize()
    assert bool((counts == -7).all())
    # mask == NULL: table 0 is the twin's result, table 1 is zero
    assert fn(*head, 0, None, 0, None, None, 0) == 0
    torch.cuda.synchronize()
    twin = ops.bilinear_bincount(z, z, w, e, precision="f32")
    assert torch.equal(counts[0], twin) and bool((counts[1] == 0).all())
    assert fn(*head, 0, None, 0, None, per.data_ptr(), words) == 0
    torch.cuda.synchronize()
    assert torch.equal(counts, ops.bilinear_bincount(z, z, w, e, precision="f32", split=per)) and torch.equal(counts.sum(0), twin)
    assert counts[1].sum(1).tolist() == [1, 1]
    # no pair at all, no outcome at all
    out = ops.bilinear_bincount(z[:0], z, w, e, split=ops.pair_mask([], [], 0, n))
    assert out.shape == (2, 2, B + 1) and bool((out == 0).all())
    out = ops.bilinear_bincount(z, z[:0], w, e, split=ops.pair_mask([], [], n, 0))
    assert out.shape == (2, 2, B + 1) and bool((out == 0).all())
    out = ops.bilinear_bincount(z, z, w[:0], e[:0], split=ops.pair_mask([], [], n, n))
    assert out.shape == (2, 0, B + 1)
    # the Python layer refuses a mask of another shape, device or plane count
    for bad in (per.cpu(), per.long(), ops.pair_mask([], [], n, n + 64), torch.cat([per, per[:1]])):
        with pytest.raises(ValueError, match="exclude"):
            ops.bilinear_bincount(z, z, w, e, split=bad)


# ------------------------------------------------------------------------------------------------ pipeline level
class _DecoderOnly(torch.nn.Module):
    """Decoder-only stand-in for NovelDDIMultilabel: the screening functions read ``model.decoder`` only."""

    def __init__(self, M, n_out, seed):
        super().__init__()
        self.decoder = M.BilinearDDIScorer(128, 128, n_out)
        torch.nn.utils.parametrize.register_parametrization(self.decoder, "weight", M.Symmetric())
        with torch.no_grad():
            self.decoder.parametrizations.weight.original.copy_(
                torch.randn(n_out, 128, 128, generator=torch.Generator().manual_seed(seed)) / 128 ** 0.5)


N_DRUGS = 300


@pytest.fixture(scope="module", params=["f32", "bf16x3"])
def case(request):
    """(prec, model, z, lower-triangle values [L, M], {planes: (known mask, class flags [L, M])}): the dense reference is the
    GENERAL sweep (the symmetric sweep switched off, as in test_bincount_gpu._case); the known network is 600 random pairs, once
    under every outcome (one plane) and once spread over the outcomes (one plane each)."""
    from madrigal_amd import models as M, ops
    from madrigal_amd._lib import lib
    from madrigal_amd.pipeline import known_pairs_mask, score_all_pairs
    prec = request.param
    model = _DecoderOnly(M, L, 0).cuda().eval()
    z = torch.randn((N_DRUGS, 128), generator=torch.Generator().manual_seed(100)).cuda()
    with pytest.MonkeyPatch.context() as mp, M.precision(prec):
        mp.setenv("MDG_BILINEAR_SYMMETRIC", "0")
        lib().mdg_tuning_reload()
        dense = score_all_pairs(model, z).contiguous()
    lib().mdg_tuning_reload()
    ii, jj = torch.tril_indices(N_DRUGS, N_DRUGS, -1, device="cuda")
    vals = dense[:, ii, jj].contiguous()
    g = torch.Generator().manual_seed(21)
    h, t = torch.randint(0, N_DRUGS, (600,), generator=g), torch.randint(0, N_DRUGS, (600,), generator=g)      # either order, some h == t
    lab = torch.randint(0, L, (600,), generator=g)
    known = {}
    for planes, mask in ((1, known_pairs_mask(N_DRUGS, h, t)), (L, known_pairs_mask(N_DRUGS, h, t, labels=lab, n_labels=L))):
        flags = ops.pair_mask_dense(mask, N_DRUGS, N_DRUGS)[:, ii, jj]
        known[planes] = (mask, flags.expand(L, -1) if planes == 1 else flags)
    return prec, model, z, vals, known


def _less_per_class(vals, flags, q):
    """int64 [2, L, Q]: per class, the number of values strictly below every query (brute_less)."""
    out = torch.empty((2,) + tuple(q.shape), dtype=torch.int64, device=vals.device)
    for l in range(vals.shape[0]):
        for p in (0, 1):
            out[p, l] = brute_less(vals[l][flags[l] == bool(p)][None, :], q[l:l + 1])[0]
    return out


@pytest.mark.parametrize("planes", [1, L])
def test_count_below_with_known_equals_brute_force_per_class(case, ops, planes):
    """Q = 2 max_edges + 5 unsorted queries with duplicates (three sweeps): per class the exact number of lower-triangle scores below
    each; the classes add up to the call without ``known``, which is unchanged; label_range slices a per-outcome mask."""
    from madrigal_amd import models as M
    from madrigal_amd.pipeline import count_below
    prec, model, z, vals, known = case
    mask, flags = known[planes]
    mx = ops.bilinear_bincount_max_edges()
    g = torch.Generator().manual_seed(11)
    real = vals[:, torch.randperm(vals.shape[1], generator=g)[:400].cuda()]               # queries that ARE scores: the < boundary
    free = (torch.randn((L, 2 * mx + 1 - 400), generator=g) * float(vals.std())).cuda()
    q = torch.cat([real, free], 1)
    q = torch.cat([q, q[:, [3, 3, 700, 2 * mx]]], 1)                                     # duplicates
    q = q[:, torch.randperm(q.shape[1], generator=g).cuda()].contiguous()
    assert q.shape == (L, 2 * mx + 5)
    with M.precision(prec):
        got = count_below(model, z, q, known=mask)
        plain = count_below(model, z, q)
        none = count_below(model, z, q, known=None)
        part = count_below(model, z, q[1:3], label_range=(1, 3), known=mask)
    assert got.shape == (2, L, q.shape[1]) and got.dtype == torch.int64
    assert torch.equal(got, _less_per_class(vals, flags, q))
    assert plain.shape == q.shape and torch.equal(plain, brute_less(vals, q)) and torch.equal(none, plain)
    assert torch.equal(got.sum(0), plain)
    assert torch.equal(part, got[:, 1:3])


def _exact_auroc(v, pos):
    """Rank-sum AUROC with ties counted 1/2 of one outcome's values, the flagged ones as positives (float64 compares)."""
    p, n = v[pos].double(), torch.sort(v[~pos].double()).values
    less = torch.searchsorted(n, p, right=False)
    eq = torch.searchsorted(n, p, right=True) - less
    return (float(less.sum()) + 0.5 * float(eq.sum())) / (p.numel() * n.numel())


@pytest.mark.parametrize("planes", [1, L])
def test_recovery_at_cuts_and_auroc_bounds_equal_the_dense_tensor(case, ops, planes):
    from madrigal_amd import models as M
    from madrigal_amd.pipeline import auroc_bounds, recovery_at_cuts, score_histogram, top_pairs
    prec, model, z, vals, known = case
    mask, flags = known[planes]
    total = vals.shape[1]
    with M.precision(prec):
        cuts = top_pairs(model, z, 50)[0].contiguous()                       # [L, 50], descending: unsorted for the sweep
        rec = recovery_at_cuts(model, z, mask, cuts)
        rec_part = recovery_at_cuts(model, z, mask, cuts[1:3], label_range=(1, 3))
        edges = torch.linspace(float(vals.min()) - 0.5, float(vals.max()) + 0.5, 1000, device="cuda")
        lower, upper = auroc_bounds(model, z, mask, edges)
        lower_part, upper_part = auroc_bounds(model, z, mask, edges, label_range=(1, 3))
        hist = score_histogram(model, z, edges)
        hist_none = score_histogram(model, z, edges, known=None)
        hist_split = score_histogram(model, z, edges, known=mask)
        w = model.decoder.symmetric_weight()
        today = ops.bilinear_bincount(z, z, w, edges[None, :].expand(L, -1).contiguous(), eligible="lower", precision=prec)
    sel = vals[:, None, :] >= cuts[:, :, None]                              # [L, 50, M]
    selected = sel.sum(2)
    hits = (sel & flags[:, None, :]).sum(2)
    n_known = flags.sum(1, keepdim=True)
    assert bool((selected >= torch.arange(1, 51, device="cuda")[None, :]).all())      # the K-th best value selects at least K pairs
    assert rec["selected"].dtype == torch.int64 and torch.equal(rec["selected"], selected) and torch.equal(rec["hits"], hits)
    precision = hits.double() / selected.double()
    for key, ref in (("precision", precision), ("recall", hits.double() / n_known.double()),
                     ("enrichment", precision / (n_known.double() / total))):
        assert rec[key].dtype == torch.float64 and torch.allclose(rec[key], ref, rtol=1e-15, atol=0), key
    for key in rec:
        assert torch.equal(rec_part[key], rec[key][1:3]), key
    # AUROC over the whole pair universe: the bounds bracket the dense rank-sum value, outcome by outcome
    assert lower.dtype == torch.float64 and lower.shape == (L,)
    for l in range(L):
        exact = _exact_auroc(vals[l], flags[l])
        print(prec, planes, l, "auroc", float(lower[l]), exact, float(upper[l]))
        assert float(lower[l]) <= exact <= float(upper[l])
        # the interval is the share of (known, novel) pairs inside one bin: at most the fullest bin's share of the novel pairs
        assert float(upper[l] - lower[l]) <= float(hist_split[0, l].max()) / float(hist_split[0, l].sum()) + 1e-15
    assert torch.equal(lower_part, lower[1:3]) and torch.equal(upper_part, upper[1:3])
    # without ``known`` the histogram is today's; with it the two classes add up to it
    assert torch.equal(hist, today) and torch.equal(hist_none, today)
    assert hist_split.shape == (2, L, 1001) and torch.equal(hist_split.sum(0), today)
    assert torch.equal(hist_split[1].sum(1), n_known[:, 0])
