"""The counting product of the all-pairs head on the GPU: mdg_bilinear_bincount against torch.bucketize + bincount of the
project's own dense head (exactly, in the fp32-grade modes), and the pipeline products built on it (count_below,
normalized_ranks_of, pair_ranks, ensemble_pair_ranks, score_histogram) against ops.rank_normalize over the dense scores."""
import pytest
import torch

from bincount_ref import brute_counts, brute_less, eligible_scores, inputs, is_unique

pytestmark = pytest.mark.gpu

ALL_ONLY = [(1, 1), (33, 4), (300, 333)]
SQUARE = [(300, 300), (513, 513)]          # past a 256-row and a 512-row workgroup, ending on a ragged 64-column tile


@pytest.fixture(scope="module")
def ops():
    from madrigal_amd import ops as _ops
    return _ops


def _modes(nh, nt):
    return ["all", "not_self", "lower"] if (nh, nt) in SQUARE else ["all"]


def _edge_sets(dense, eligible, max_edges):
    """{name: edges [L, B]}: one edge at 0; 37 edges that ARE eligible scores of the outcome, one of them twice (the < / <=
    boundary and an empty bin on real values); max_edges edges past both extremes; all edges below the minimum; all above
    the maximum (each fast path alone)."""
    vals = eligible_scores(dense, eligible)
    L, M = vals.shape
    lo, hi = float(vals.min()), float(vals.max())
    pick = torch.randint(0, M, (L, 37), generator=torch.Generator().manual_seed(7)).to(vals.device)
    real = torch.sort(torch.gather(vals, 1, pick), dim=1).values
    real[:, 11] = real[:, 10]
    line = lambda a, b, n: torch.linspace(a, b, n, device=vals.device)[None, :].expand(L, -1).contiguous()   # noqa: E731
    return {"zero": torch.zeros((L, 1), device=vals.device), "real": real.contiguous(), "wide": line(lo - 1, hi + 1, max_edges),
            "below": line(lo - 3, lo - 1, 5), "above": line(hi + 1, hi + 3, 5)}, M


@pytest.mark.parametrize("nh,nt", ALL_ONLY + SQUARE)
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_counts_equal_bucketize_of_the_dense_general_sweep(ops, prec, nh, nt):
    """counts == torch.bucketize(right=True) + bincount of the eligible entries of the STORE tensor of the general sweep in the
    same precision, every eligibility mode and edge set; every row sums to the number of eligible pairs."""
    L = 3
    zh, zt, w = inputs(nh, nt, L)
    zh, zt, ws = zh.cuda(), zt.cuda(), ops.symmetrize(w.cuda())
    dense = ops.bilinear_allpairs(zh, zt, ws, precision=prec)
    for eligible in _modes(nh, nt):
        sets, M = _edge_sets(dense, eligible, ops.bilinear_bincount_max_edges())
        for name, e in sets.items():
            counts = ops.bilinear_bincount(zh, zt, ws, e, eligible=eligible, precision=prec)
            assert counts.shape == (L, e.shape[1] + 1) and counts.dtype == torch.int64
            ref = brute_counts(dense, e, eligible)
            assert torch.equal(counts, ref), (eligible, name, (counts - ref).abs().sum().item())
            assert bool((counts.sum(1) == M).all()), (eligible, name)
            if name == "real":
                assert bool((counts[:, 11] == 0).all())                       # between the two equal edges
                assert torch.equal(ops.bilinear_bincount(zh, zt, ws, e, eligible=eligible, precision=prec), counts)


@pytest.mark.parametrize("nh,nt", SQUARE)
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_counts_of_the_16bit_sweeps_are_within_the_regrouping_bound(ops, prec, nh, nt):
    """The single-product modes run the row-statistics sweep (16x16x32: fp32 sums grouped differently from the dense 32x32x16
    sweep, <= 2e-6 of the scale): for every edge e the cumulative count C(e) lies between the dense counts below e - delta and
    below e + delta, delta = 2e-6 max|dense|; the total is exact."""
    L = 3
    zh, zt, w = inputs(nh, nt, L)
    zh, zt, ws = zh.cuda(), zt.cuda(), ops.symmetrize(w.cuda())
    dense = ops.bilinear_allpairs(zh, zt, ws, precision=prec)
    delta = 2e-6 * float(dense.abs().max())
    for eligible in _modes(nh, nt):
        vals = eligible_scores(dense, eligible)
        sets, M = _edge_sets(dense, eligible, ops.bilinear_bincount_max_edges())
        for name, e in sets.items():
            counts = ops.bilinear_bincount(zh, zt, ws, e, eligible=eligible, precision=prec)
            assert bool((counts.sum(1) == M).all()), (eligible, name)
            C = torch.cumsum(counts, 1)[:, :-1]
            lo, hi = brute_less(vals, e, -delta), brute_less(vals, e, delta)
            print(prec, (nh, nt), eligible, name, "max C - lo", int((C - lo).max()), "max hi - C", int((hi - C).max()),
                  "min", int((C - lo).min()), int((hi - C).min()))
            assert bool((lo <= C).all()) and bool((C <= hi).all()), (eligible, name)


def test_c_level_refusals_launch_nothing(ops):
    from madrigal_amd._lib import lib
    z = torch.randn(6, 128, device="cuda")
    w = torch.randn(2, 128, 128, device="cuda")
    mx = ops.bilinear_bincount_max_edges()
    e = torch.zeros(2, mx + 1, device="cuda")
    counts = torch.full((2, mx + 2), -7, dtype=torch.int64, device="cuda")
    for nt, B, el, what in ((6, mx + 1, 0, b"n_edges"), (4, 3, 2, b"one drug set"), (4, 3, 1, b"one drug set"), (6, 3, 9, b"eligible")):
        rc = lib().mdg_bilinear_bincount(z.data_ptr(), z.data_ptr(), w.data_ptr(), e.data_ptr(), counts.data_ptr(), 6, nt, 2, 128, B, 0, el,
                                         None, 0, None)
        assert rc != 0 and b"mdg_bilinear_bincount" in lib().mdg_last_error() and what in lib().mdg_last_error()
    # bf16x3 needs the operand images: refused without a workspace, before anything is enqueued
    rc = lib().mdg_bilinear_bincount(z.data_ptr(), z.data_ptr(), w.data_ptr(), e.data_ptr(), counts.data_ptr(), 6, 6, 2, 128, 3, 1, 0, None, 0, None)
    assert rc == -2 and b"workspace" in lib().mdg_last_error()
    torch.cuda.synchronize()
    assert bool((counts == -7).all())
    # no pair at all: zero counts
    out = ops.bilinear_bincount(z[:0], z, w, e[:, :3].contiguous())
    assert out.shape == (2, 4) and bool((out == 0).all())
    out = ops.bilinear_bincount(z, z, w[:0], e[:0, :3].contiguous())
    assert out.shape == (0, 4)
    with pytest.raises(ValueError, match="ascending"):
        ops.bilinear_bincount(z, z, w, torch.tensor([[1.0, 0.0]] * 2, device="cuda"))


# ------------------------------------------------------------------------------------------------ pipeline level
class _DecoderOnly(torch.nn.Module):
    """Decoder-only stand-in for NovelDDIMultilabel: the screening functions read ``model.decoder`` only."""

    def __init__(self, M, L, seed):
        super().__init__()
        self.decoder = M.BilinearDDIScorer(128, 128, L)
        torch.nn.utils.parametrize.register_parametrization(self.decoder, "weight", M.Symmetric())
        with torch.no_grad():
            self.decoder.parametrizations.weight.original.copy_(
                torch.randn(L, 128, 128, generator=torch.Generator().manual_seed(seed)) / 128 ** 0.5)


N_DRUGS, N_OUT = 300, 3


def _case(prec, seed):
    """(model, z, dense, ranks) of one checkpoint: ``dense`` = score_all_pairs(model, z) and ``ranks`` =
    ops.rank_normalize(dense), with the head's symmetric sweep switched off.  The counting sweep follows the GENERAL sweep
    (S[l,i,j] = (z_i W) z_j, what top_pairs / top_partners report); the symmetric sweep fills the lower triangle outside its
    256 x 256 diagonal blocks with the mirrored (z_j W) z_i, and runs bf16x3 on another MFMA shape: its scores differ from the
    general sweep's in the last bits, so ranks taken over it differ by a few places wherever two scores are that close."""
    from madrigal_amd import models as M, ops
    from madrigal_amd._lib import lib
    from madrigal_amd.pipeline import score_all_pairs
    model = _DecoderOnly(M, N_OUT, seed).cuda().eval()
    z = torch.randn((N_DRUGS, 128), generator=torch.Generator().manual_seed(100 + seed)).cuda()
    with pytest.MonkeyPatch.context() as mp, M.precision(prec):
        mp.setenv("MDG_BILINEAR_SYMMETRIC", "0")
        lib().mdg_tuning_reload()
        dense = score_all_pairs(model, z).contiguous()
        with torch.no_grad():
            assert torch.equal(dense, model.decoder(z.clone(), z))            # the general sweep
        ranks = ops.rank_normalize(dense).contiguous()
    lib().mdg_tuning_reload()
    return model, z, dense, ranks


@pytest.fixture(scope="module", params=["f32", "bf16x3"])
def case(request):
    return (request.param,) + _case(request.param, 0)


def _lower(dense):
    N = dense.shape[1]
    ii, jj = torch.tril_indices(N, N, -1, device=dense.device)
    return ii, jj, dense[:, ii, jj]


def test_count_below_equals_brute_force_over_three_edge_chunks(case, ops, monkeypatch):
    """Q = 2 max_edges + 5 unsorted queries with duplicates: three sweeps, the exact number of lower-triangle scores below each."""
    from madrigal_amd import models as M
    from madrigal_amd.pipeline import count_below
    prec, model, z, dense, _ = case
    mx = ops.bilinear_bincount_max_edges()
    _, _, vals = _lower(dense)
    g = torch.Generator().manual_seed(11)
    real = vals[:, torch.randperm(vals.shape[1], generator=g)[:400].cuda()]               # queries that ARE scores: the < boundary
    free = (torch.randn((N_OUT, 2 * mx + 1 - 400), generator=g) * float(vals.std())).cuda()
    q = torch.cat([real, free], 1)
    q = torch.cat([q, q[:, [3, 3, 700, 2 * mx]]], 1)                                     # duplicates
    q = q[:, torch.randperm(q.shape[1], generator=g).cuda()].contiguous()
    assert q.shape == (N_OUT, 2 * mx + 5)
    assert min(int(torch.unique(q[l]).numel()) for l in range(N_OUT)) > 2 * mx          # distinct values: more than two chunks
    sweeps = []
    inner = model.decoder.bincount
    monkeypatch.setattr(model.decoder, "bincount", lambda *a, **k: (sweeps.append(a[2].shape), inner(*a, **k))[1])
    with M.precision(prec):
        less = count_below(model, z, q)
        part = count_below(model, z, q[1:3], label_range=(1, 3))
    assert len(sweeps) == 6 and sweeps[0][1] == mx
    assert less.dtype == torch.int64 and torch.equal(less, brute_less(vals, q))
    assert torch.equal(part, less[1:3])
    with pytest.raises(ValueError, match="finite"):
        count_below(model, z, torch.full((N_OUT, 2), float("nan"), device="cuda"))


def _assert_ranks(got, ref, vals, q, what):
    """Bit-equal wherever the query's score is unique in its outcome; at most 1 % of the queries are left out as tied."""
    uniq = is_unique(vals, q)
    out = 1.0 - float(uniq.float().mean())
    print(what, "queries", q.numel(), "left out as tied", int((~uniq).sum()), "differing", int((got[uniq] != ref[uniq]).sum()))
    assert out <= 0.01, out
    assert torch.equal(got[uniq], ref[uniq]), what


def test_normalized_ranks_of_equal_the_rank_tensor(case, monkeypatch):
    """normalized_ranks_of(scores) == ops.rank_normalize(score_all_pairs(model, z)) at the pairs that carry those scores: the
    top_pairs(K = 50) values and 200 lower-triangle entries drawn with a fixed seed."""
    from madrigal_amd import models as M, ops
    from madrigal_amd.pipeline import normalized_ranks_of, score_all_pairs, top_pairs
    prec, model, z, dense, ranks = case
    ii, jj, vals = _lower(dense)
    with M.precision(prec):
        v, h, t = top_pairs(model, z, 50)
        draw = torch.randperm(vals.shape[1], generator=torch.Generator().manual_seed(5))[:200].cuda()
        q = torch.cat([v, vals[:, draw]], 1).contiguous()
        ref = torch.cat([ranks[torch.arange(N_OUT, device="cuda")[:, None], h, t], ranks[:, ii[draw], jj[draw]]], 1)
        got = normalized_ranks_of(model, z, q)
        assert got.dtype == torch.float32 and got.shape == q.shape
        _assert_ranks(got, ref, vals, q, f"normalized_ranks_of {prec}")
        # for the record (no assertion): the same entries of the ranks taken over the SYMMETRIC sweep's tensor
        sym = ops.rank_normalize(score_all_pairs(model, z))
        ref_sym = torch.cat([sym[torch.arange(N_OUT, device="cuda")[:, None], h, t], sym[:, ii[draw], jj[draw]]], 1)
        print("against the symmetric sweep's rank tensor:", int((got != ref_sym).sum()), "of", got.numel(), "entries differ")


def test_pair_ranks_and_their_ensemble(case):
    """pair_ranks of pairs given in both orders and of the top_partners(k = 4) hit lists == the dense score and the rank tensor's
    entry at [l, max(i, j), min(i, j)]; ensemble_pair_ranks of two checkpoints == ops.gmean of the two."""
    from madrigal_amd import models as M, ops
    from madrigal_amd.pipeline import ensemble_pair_ranks, pair_ranks, top_partners
    prec, model, z, dense, ranks = case
    _, _, vals = _lower(dense)
    with M.precision(prec):
        pv, pi = top_partners(model, z, 4)
        rows = torch.arange(20, device="cuda")
        hit_h = rows[None, :, None].expand(N_OUT, -1, 4).reshape(-1)
        hit_t = pi[:, :20].reshape(-1).long()
        heads = torch.cat([torch.tensor([5, 2, 299, 0, 150, 7], device="cuda"), hit_h])
        tails = torch.cat([torch.tensor([2, 5, 0, 299, 7, 150], device="cuda"), hit_t])
        big, small = torch.maximum(heads, tails), torch.minimum(heads, tails)
        for budget in (1 << 30, 8 * N_DRUGS * 4):                      # one chunk; eight rows and one outcome per chunk
            s, r = pair_ranks(model, z, heads.tolist() if budget < 1 << 30 else heads, tails, max_temp_bytes=budget)
            assert s.shape == (N_OUT, heads.numel()) and r.shape == s.shape and r.dtype == torch.float32
            assert torch.equal(s, dense[:, big, small])
            _assert_ranks(r, ranks[:, big, small], vals, s, f"pair_ranks {prec}")
        assert torch.equal(s[:, :3], s[:, [1, 0, 3]]) and torch.equal(r[:, 4], r[:, 5])      # either order, one pair
        # a top_partners hit with j < i carries S[l, i, j] itself
        own = torch.arange(N_OUT, device="cuda").repeat_interleave(80)
        low = hit_t < hit_h
        assert torch.equal(s[own, 6 + torch.arange(240, device="cuda")][low], pv[:, :20].reshape(-1)[low])
        s2, r2 = pair_ranks(model, z, heads, tails, label_range=(1, 3))
        assert torch.equal(s2, s[1:3]) and torch.equal(r2, r[1:3])
        with pytest.raises(ValueError, match="itself"):
            pair_ranks(model, z, [1, 4], [2, 4])
        with pytest.raises(ValueError):
            pair_ranks(model, z, [1, N_DRUGS], [2, 3])
        model_b, z_b, dense_b, ranks_b = _case(prec, 1)
        per, gm = ensemble_pair_ranks([model, model_b], [z, z_b], heads, tails)
        r_b = pair_ranks(model_b, z_b, heads, tails)[1]
        assert per.shape == (2, N_OUT, heads.numel()) and torch.equal(per[0], r) and torch.equal(per[1], r_b)
        _assert_ranks(r_b, ranks_b[:, big, small], _lower(dense_b)[2], dense_b[:, big, small], f"ensemble member {prec}")
        assert gm.shape == r.shape and torch.equal(gm, ops.gmean([r, r_b]))
        both = (per[0] > 0) & (per[1] > 0)
        assert torch.allclose(gm[both], (per[0][both].double() * per[1][both].double()).sqrt().float(), rtol=1e-5)


@pytest.fixture(scope="module")
def small_model():
    """A configs.build_model model (drugbank163 layout, 6 outcomes) and the embeddings of 130 drugs from generate_embeddings."""
    from madrigal_amd import configs, data as D, models as M
    from madrigal_amd.pipeline import generate_embeddings
    n, L = 130, 6
    batch, bkg = D.make_batch(n, 5, kg_nodes=900, kg_edges=6000)
    b = D.batch_to(batch, "cuda")
    kgc = {"data": bkg["data"].to("cuda"), "drug_index_map": bkg["drug_index_map"].cuda()}
    torch.manual_seed(3)
    model = configs.build_model("drugbank163", bkg["data"], L).cuda().eval()
    filler = torch.randn((n, 128), generator=torch.Generator().manual_seed(6)).cuda()
    with M.precision("bf16x3"):
        z = generate_embeddings(model, b, kgc, kg_filler=filler).contiguous()
    assert z.shape == (n, 128) and bool(torch.isfinite(z).all())
    return model, z


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_score_histogram_on_a_built_model(small_model, ops, prec):
    from madrigal_amd import models as M
    from madrigal_amd.pipeline import score_histogram
    model, z = small_model
    n = z.shape[0]
    with M.precision(prec), torch.no_grad():
        w = model.decoder.symmetric_weight()
        dense = model.decoder(z.clone(), z)                               # the general sweep
        edges = torch.linspace(float(dense.min()) - 0.5, float(dense.max()) + 0.5, 64, device="cuda")
        full = edges[None, :].expand(6, -1).contiguous()
        hist = score_histogram(model, z, edges)
        assert hist.shape == (6, 65) and bool((hist.sum(1) == n * (n - 1) // 2).all())
        assert torch.equal(hist, ops.bilinear_bincount(z, z, w, full, eligible="lower", precision=prec))
        assert torch.equal(hist, brute_counts(dense, full, "lower"))
        assert torch.equal(score_histogram(model, z, edges, label_range=(2, 5)), hist[2:5])
        per = full[2:5] + torch.tensor([[0.0], [0.25], [0.5]], device="cuda")
        assert torch.equal(score_histogram(model, z, per, label_range=(2, 5)),
                           ops.bilinear_bincount(z, z, w[2:5], per.contiguous(), eligible="lower", precision=prec))
        ns = score_histogram(model, z, edges, eligible="not_self")
        assert torch.equal(ns, brute_counts(dense, full, "not_self")) and bool((ns.sum(1) == n * (n - 1)).all())
    with pytest.raises(ValueError):
        score_histogram(model, z, full[:4])
    with pytest.raises(ValueError):
        score_histogram(model, z, edges, label_range=(0, 7))
