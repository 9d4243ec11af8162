"""The screen bodies of madrigal_amd.pipeline, which the single-model and the ensemble functions share, driven on the CPU by a head
backed by a dense [L, N, N] tensor, against brute force on that tensor: the chunking, the plane index ``s + l`` of a per-outcome
mask, the open-row re-score, the CSR expansion, the edge chunks of count_below, the row rectangle of the profile and the row
blocks of most_flagged.  N = 37 (a second word row in the packed mask), values on 8 levels (exact ties everywhere), 4 outcomes of
which the screens see [1, 4)."""
import functools

import pytest
import torch

from profile_ref import dense_profile
from test_ensemble_profile_cpu import _brute_force as most_flagged_brute_force, _lists
from test_exclude_cpu import as_mask, numpy_pack
from test_topk_cpu import brute_force_pairs

NEG = float("-inf")
N, L_ALL, RANGE = 37, 4, (1, 4)
LO, HI = RANGE


def _head_class():
    from madrigal_amd import ops, pipeline

    class DenseHead(pipeline._Head):
        """``pipeline._Head`` over a stored tensor: every product by sorting, comparing and counting its entries."""

        def __init__(self, dense):
            self.dense, self.n_outcomes, self.N, self.device = dense, dense.shape[0], dense.shape[1], dense.device
            self.edge_counts = []

        def _eligible(self, s, e, eligible, mask):
            i, j = torch.arange(self.N)[:, None], torch.arange(self.N)[None, :]
            ok = {"all": j >= 0, "not_self": j != i, "lower": j < i}[eligible].expand(e - s, -1, -1)
            planes = pipeline._planes(mask, s, e)
            return ok if planes is None else ok & ~ops.pair_mask_dense(planes, self.N, self.N)

        def topk(self, k, s, e, eligible, exclude):
            d = self.dense[s:e].masked_fill(~self._eligible(s, e, eligible, exclude), NEG)
            sv, si = torch.sort(d, dim=2, descending=True, stable=True)
            pad = max(k - self.N, 0)
            sv = torch.cat([sv[..., :k], sv.new_full((e - s, self.N, pad), NEG)], 2)
            si = torch.cat([si[..., :k], si.new_full((e - s, self.N, pad), -1)], 2)
            return sv.contiguous(), torch.where(sv == NEG, -1, si).to(torch.int32).contiguous()

        def dense_rows(self, rows, s, e):
            return self.dense[s:e, rows].clone()

        def select_count(self, thr, s, e, eligible, exclude):
            return ((self.dense[s:e] >= thr[:, None, None]) & self._eligible(s, e, eligible, exclude)).sum(2).to(torch.int32)

        def select(self, thr, s, e, eligible, max_bytes, exclude):
            hit = (self.dense[s:e] >= thr[:, None, None]) & self._eligible(s, e, eligible, exclude)
            row_ptr = torch.zeros((e - s) * self.N + 1, dtype=torch.int64)
            row_ptr[1:] = torch.cumsum(hit.sum(2).reshape(-1), 0)
            where = hit.nonzero()
            return row_ptr, where[:, 2].to(torch.int32), self.dense[s:e][hit]

        def bincount(self, edges, s, e, eligible, split):
            assert edges.is_contiguous() and edges.shape == (e - s, edges.shape[1])
            self.edge_counts.append(edges.shape[1])
            B = edges.shape[1]
            ok = self._eligible(s, e, eligible, None)
            known = None if split is None else ops.pair_mask_dense(pipeline._planes(split, s, e), self.N, self.N).expand(e - s, -1, -1)
            out = torch.zeros((2, e - s, B + 1), dtype=torch.int64)
            for l in range(e - s):
                bins = torch.bucketize(self.dense[s + l], edges[l], right=True)
                for c in range(2):
                    keep = ok[l] if known is None else ok[l] & (known[l] == bool(c))
                    out[c, l] = torch.bincount(bins[keep], minlength=B + 1)
            return out[0] if split is None else out

        def profile(self, rows, cols, thr, scale, s, e, eligible):
            d = self.dense[s:e]
            d = d if rows is None else d[:, rows]
            return dense_profile((d if cols is None else d[:, :, cols]).contiguous(), thr, scale, eligible)

    return DenseHead


@functools.lru_cache(maxsize=None)
def _setting():
    """(dense [4, N, N] on 8 levels, per-outcome known pairs bool [4, N, N] symmetric, their packed mask)."""
    g = torch.Generator().manual_seed(11)
    dense = torch.floor(torch.rand((L_ALL, N, N), generator=g) * 8) / 8
    known = torch.rand((L_ALL, N, N), generator=g) < 0.25
    known[:, N - 1, ::2] = True                                   # a hub whose best partners are mostly known, in the second word row
    known = known | known.transpose(1, 2)
    known[:, torch.arange(N), torch.arange(N)] = False
    mask = as_mask(numpy_pack(known.numpy()))
    assert mask.shape == (L_ALL, 2, 64)
    return dense, known, mask


def _lower(x):
    ii, jj = torch.tril_indices(N, N, -1)
    return x[:, ii, jj]


@pytest.mark.parametrize("max_temp_bytes", [1, 2 * N * 2 * 48, 1 << 30])      # one, two and all outcomes per chunk
@pytest.mark.parametrize("excluded", [False, True])
def test_top_pairs_with_open_rows_equals_brute_force(excluded, max_temp_bytes):
    from madrigal_amd import pipeline
    dense, known, mask = _setting()
    info = {}
    v, h, t = pipeline._top_pairs(_head_class()(dense), 60, RANGE, 2, max_temp_bytes, info, mask if excluded else None)
    ref = dense[LO:HI].masked_fill(known[LO:HI], NEG) if excluded else dense[LO:HI]
    bv, bh, bt = brute_force_pairs(ref, 60)
    assert bool((bv > NEG).all())
    assert torch.equal(v, bv) and torch.equal(h, bh) and torch.equal(t, bt)
    assert len(info["open_rows"]) == HI - LO and max(info["open_rows"]) >= 1, info      # the re-score really ran
    if excluded:
        assert not bool(known[torch.arange(LO, HI)[:, None], h, t].any())
    with pytest.raises(ValueError, match="K: expected"):
        pipeline._top_pairs(_head_class()(dense), 0, RANGE, 2, 1 << 30, None, None)
    with pytest.raises(ValueError, match="label_range"):
        pipeline._top_pairs(_head_class()(dense), 60, (1, 5), 2, 1 << 30, None, None)
    with pytest.raises(ValueError, match="exclude: 3 planes"):
        pipeline._top_pairs(_head_class()(dense), 60, RANGE, 2, 1 << 30, None, mask[:3])


def test_top_partners_picks_rows_from_outcome_chunks():
    from madrigal_amd import pipeline
    dense, known, mask = _setting()
    head = _head_class()(dense)
    vals, idx = pipeline._top_partners(head, 3, RANGE, None, 1 << 30, mask)
    d = dense[LO:HI].masked_fill(known[LO:HI] | torch.eye(N, dtype=torch.bool), NEG)
    sv, si = torch.sort(d, dim=2, descending=True, stable=True)
    assert torch.equal(vals, sv[..., :3]) and torch.equal(idx.long(), si[..., :3])
    rows = [36, 0, 36, 5]
    v2, i2 = pipeline._top_partners(head, 3, RANGE, rows, 1, mask)             # one outcome per chunk
    assert torch.equal(v2, vals[:, rows]) and torch.equal(i2, idx[:, rows])


def test_pairs_above_with_a_tied_cut_an_empty_outcome_and_no_drug():
    from madrigal_amd import pipeline
    dense, known, mask = _setting()
    thr = torch.tensor([0.75, 2.0, 0.875])                               # on a level: ties are selected; nothing; the top level
    for excl in (None, mask):
        offsets, h, t, vals = pipeline._pairs_above(_head_class()(dense), thr, RANGE, 1 << 30, excl)
        sizes = []
        for l in range(LO, HI):
            keep = _lower(dense)[l] >= thr[l - LO]
            if excl is not None:
                keep &= ~_lower(known)[l]
            ii, jj = torch.tril_indices(N, N, -1)
            a, b = int(offsets[l - LO]), int(offsets[l - LO + 1])
            assert torch.equal(h[a:b], ii[keep]) and torch.equal(t[a:b], jj[keep]) and torch.equal(vals[a:b], _lower(dense)[l][keep])
            sizes.append(b - a)
        assert sizes[0] > 0 and sizes[1] == 0 and sizes[2] > 0 and int(offsets[-1]) == h.numel()
        assert bool((vals[: sizes[0]] == 0.75).any())
    counts = pipeline._partner_counts(_head_class()(dense), thr, RANGE, None)
    want = ((dense[LO:HI] >= thr[:, None, None]) & ~torch.eye(N, dtype=torch.bool)).sum(2)
    assert counts.dtype == torch.int32 and torch.equal(counts.long(), want)
    offsets, h, t, vals = pipeline._pairs_above(_head_class()(dense[:, :0, :0]), 0.5, RANGE, 1 << 30, None)
    assert offsets.tolist() == [0, 0, 0, 0] and h.numel() == t.numel() == vals.numel() == 0
    with pytest.raises(ValueError, match="thresholds"):
        pipeline._pairs_above(_head_class()(dense), thr[:2], RANGE, 1 << 30, None)


def test_count_below_and_recovery_over_several_edge_chunks(monkeypatch):
    from madrigal_amd import ops, pipeline
    dense, known, mask = _setting()
    monkeypatch.setattr(ops, "bilinear_bincount_max_edges", lambda: 4)
    levels = torch.arange(9.0) / 8                                        # every level, the values between them, repeats, unsorted
    q = torch.cat([levels, levels[:6] + 1 / 16, levels[2:5]])[torch.randperm(18, generator=torch.Generator().manual_seed(3))]
    q = torch.stack([q, q.flip(0), q.roll(5)])
    vals, cls = _lower(dense)[LO:HI], _lower(known)[LO:HI]
    below = vals[:, None, :] < q[:, :, None]                               # [L', Q, pairs]
    head = _head_class()(dense)
    assert torch.equal(pipeline._count_below(head, q, RANGE, None)[0], below.sum(2))
    assert head.edge_counts == [4, 4, 4, 3]                                # 15 distinct values, four at a time
    less, totals = pipeline._count_below(head, q, RANGE, mask)
    assert torch.equal(less[1], (below & cls[:, None, :]).sum(2)) and torch.equal(less[0], (below & ~cls[:, None, :]).sum(2))
    assert torch.equal(totals[1], cls.sum(1)) and torch.equal(totals[0], (~cls).sum(1))
    rec = pipeline._recovery_at_cuts(head, mask, q, RANGE)
    selected, hits = (~below).sum(2), (~below & cls[:, None, :]).sum(2)
    assert torch.equal(rec["selected"], selected) and torch.equal(rec["hits"], hits)
    assert torch.equal(rec["recall"], hits.double() / cls.sum(1)[:, None].double())
    precision = torch.where(selected == 0, torch.full(selected.shape, float("nan"), dtype=torch.float64), hits.double() / selected.double())
    assert torch.equal(rec["precision"].nan_to_num(-1.0), precision.nan_to_num(-1.0)) and bool((selected == 0).any())
    hist = pipeline._score_histogram(head, levels[1:5], RANGE, "lower", mask)
    assert hist.shape == (2, 3, 5) and torch.equal(hist.sum((0, 2)), torch.full((3,), N * (N - 1) // 2))
    lower, upper = pipeline._auroc_bounds(head, mask, levels[1:5], RANGE)
    assert bool((lower <= upper).all())
    with pytest.raises(ValueError, match="known: expected a mask"):
        pipeline._recovery_at_cuts(head, None, q, RANGE)
    with pytest.raises(ValueError, match="cuts: expected"):
        pipeline._recovery_at_cuts(head, mask, q[:2], RANGE)
    with pytest.raises(ValueError, match="scores: expected"):
        pipeline._count_below(head, q[0], RANGE, None)


def test_outcome_profile_of_a_row_rectangle_in_the_lower_triangle():
    from madrigal_amd import pipeline
    dense, known, mask = _setting()
    thr, scale = torch.tensor([0.5, 0.25, 0.75]), torch.tensor([1.0, 2.0, 0.5])
    for chunk in (65535, 2):                                               # one sweep, and two merged
        count, best, margin = pipeline._outcome_profile(_head_class()(dense), thr, scale, RANGE, "lower", (5, 20), chunk)
        rc, rb, rm = dense_profile(dense[LO:HI], thr, scale, "lower")
        assert count.shape == (15, N) and best.dtype == torch.int64
        assert torch.equal(count, rc[5:20]) and torch.equal(margin, rm[5:20])
        assert torch.equal(best, torch.where(rb[5:20] >= 0, rb[5:20].long() + LO, -1)) and int(best.max()) >= LO + 1
    shared = mask[2:3]
    count, best, margin = pipeline._outcome_profile(_head_class()(dense), thr, scale, RANGE, "not_self", None, 65535, shared)
    rc, rb, rm = dense_profile(dense[LO:HI], thr, scale, "not_self")
    assert torch.equal(count, rc.masked_fill(known[2], 0)) and torch.equal(margin, rm.masked_fill(known[2], NEG))
    assert torch.equal(best, torch.where(rb >= 0, rb.long() + LO, -1).masked_fill(known[2], -1))
    with pytest.raises(ValueError, match="out of scope"):
        pipeline._outcome_profile(_head_class()(dense), thr, scale, RANGE, "lower", None, 65535, mask)


def test_most_flagged_over_three_row_blocks_with_a_tie_at_the_last_place():
    from madrigal_amd import pipeline
    dense, known, mask = _setting()
    thr, scale = torch.full((3,), 0.5), torch.tensor([1.0, 2.0, 0.5])
    everything = most_flagged_brute_force(dense[LO:HI], thr, scale, N * (N - 1) // 2, lo=LO)
    keys = list(zip(everything[0], everything[4]))
    K = next(k for k in range(20, len(keys)) if keys[k - 1] == keys[k])    # the K-th and the next pair tie in count and margin
    blocks = []
    head = _head_class()(dense)
    inner = head.profile
    head.profile = lambda rows, cols, *a: (blocks.append((rows.start, rows.stop, cols.stop)), inner(rows, cols, *a))[1]
    got = _lists(pipeline._most_flagged_pairs(head, thr, K, scale, RANGE, 48 * N * 12, None))
    assert got == most_flagged_brute_force(dense[LO:HI], thr, scale, K, lo=LO)
    assert blocks == [(1, 13, 13), (13, 25, 25), (25, 37, 37)]
    got = _lists(pipeline._most_flagged_pairs(head, thr, K, scale, RANGE, 48 * N * 12, mask[2:3]))
    assert got == most_flagged_brute_force(dense[LO:HI], thr, scale, K, lo=LO, removed=known[2])
    with pytest.raises(ValueError, match="K: expected"):
        pipeline._most_flagged_pairs(head, thr, True, scale, RANGE, 1 << 30, None)


@pytest.mark.parametrize("attr", ["N", "device", "n_outcomes", "ws", "prec"])
def test_the_ensemble_head_checks_its_operands_at_the_first_read_of_any_attribute(attr):
    from madrigal_amd import pipeline
    with pytest.raises(ValueError, match="some_screen: 1..8 models"):
        getattr(pipeline._EnsembleHead([], [], "some_screen"), attr)
    with pytest.raises(ValueError, match="GPU"):
        getattr(pipeline._EnsembleHead([torch.zeros(2, 4, 4)], [torch.zeros(3, 4)], "some_screen"), attr)
    with pytest.raises(AttributeError):
        pipeline._EnsembleHead([], [], "some_screen").no_such_thing
