"""On-device k-nearest-neighbour search and the kNN classifier (csrc/knn.hip, ops.knn_topk / knn_vote, retrieval.nearest_neighbors /
inst_dist_topk_indices / knn_classifier / knn_predict, pipeline.similar_drugs) against the fp64 restatement tests/knn_ref.py, the
existing match-count sweep and the reference's recorded accuracies (tests/golden/knn.npz)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_ref as R                                              # noqa: E402
from test_knn_cpu import CLASSES, KS, METRICS, TS, case_key      # noqa: E402

pytestmark = pytest.mark.gpu

TOL = R.TOL                                                       # 1e-5: above the fp32 bound 128 * 2^-24 of a 128-term dot product


def _cuda(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()


def _knn(Q, L, k, metric, skip=None, segments=None):
    from madrigal_amd import ops
    sk = None if skip is None else _cuda(skip, torch.int32)
    vals, idx = ops.knn_topk(_cuda(Q), _cuda(L), k, metric=metric, skip=sk, segments=segments)
    assert vals.dtype == torch.float32 and idx.dtype == torch.int32 and vals.shape == idx.shape == (Q.shape[0], k)
    return vals.cpu().numpy(), idx.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _integers(nq, nl, seed=0):
    """Entries in {-2..2}: every dot product and squared distance is an exact fp32 integer and ties are abundant; a quarter of the
    library rows are copies of other rows, and some queries are library rows."""
    rng = np.random.default_rng([seed, nq, nl])
    L = rng.integers(-2, 3, (nl, 128)).astype(np.float32)
    dup = rng.integers(0, nl, max(nl // 4, 1))
    L[dup] = L[rng.integers(0, nl, dup.size)]
    Q = rng.integers(-2, 3, (nq, 128)).astype(np.float32)
    own = rng.integers(0, nq, max(nq // 3, 1))
    Q[own] = L[rng.integers(0, nl, own.size)]
    return Q, L


@functools.lru_cache(maxsize=None)
def _reals(nq, nl, seed=0):
    """Real-valued inputs (rows of uneven length) whose order-ambiguous queries at k = 1, 5, 20 (tol 1e-5, every metric) were
    redrawn, and the three rankings of the final draw."""
    rng = np.random.default_rng([seed, nq, nl, 5])
    draw = lambda n: (rng.standard_normal((n, 128)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    L, Q = draw(nl), draw(nq)
    rows = np.arange(nq)
    for _ in range(50):
        bad = np.zeros(rows.size, dtype=bool)
        for metric in R.METRICS:
            rk = R.Ranked(Q[rows], L, metric)
            for k in KS:
                if k <= nl:
                    bad[rk.ambiguous(k, TOL, order=True)] = True
        rows = rows[bad]
        if rows.size == 0:
            break
        Q[rows] = draw(rows.size)
    assert rows.size == 0
    return Q, L, {metric: R.Ranked(Q, L, metric) for metric in R.METRICS}


# ------------------------------------------------------------------------------------------ 1. exact integers and ties
@pytest.mark.parametrize("metric", ["dot", "euclidean"])
@pytest.mark.parametrize("nl", [1, 5, 127, 129, 300, 1000])
def test_integer_inputs_match_exactly(nl, metric):
    for nq in (1, 31, 33, 129):
        Q, L = _integers(nq, nl)
        rk = R.Ranked(Q, L, metric)
        for k in (1, 5, 20, 32):
            if k > nl:
                continue
            want_v, want_i = rk.topk(k)
            got_v, got_i = _knn(Q, L, k, metric)
            assert 0 <= got_i.min() and got_i.max() < nl                          # a clamped padding column never appears
            assert np.array_equal(got_i, want_i), (nq, k, np.flatnonzero((got_i != want_i).any(1))[:5])
            assert np.array_equal(got_v, want_v.astype(np.float32)), (nq, k)


# ------------------------------------------------------------------------------------------ 2. column segments
@pytest.mark.parametrize("kind", ["integers", "reals"])
def test_segments_are_bit_identical(kind):
    from madrigal_amd import ops
    nq, nl, k = 77, 1000, 20
    Q, L = _integers(nq, nl) if kind == "integers" else _reals(nq, nl, seed=1)[:2]
    assert ops.knn_default_segments(nq, nl) == 8
    for metric in R.METRICS:
        base_v, base_i = _knn(Q, L, k, metric, segments=1)
        for segments in (2, 3, 8, None):
            v, i = _knn(Q, L, k, metric, segments=segments)
            assert np.array_equal(i, base_i), (metric, segments)
            assert np.array_equal(v.view(np.int32), base_v.view(np.int32)), (metric, segments)


# ------------------------------------------------------------------------------------------ 3. real values against fp64
@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("nq,nl", [(77, 300), (257, 1000), (1000, 4099)])
def test_real_inputs_against_fp64(nq, nl, metric):
    Q, L, ranked = _reals(nq, nl)
    rk = ranked[metric]
    rows = np.arange(nq)[:, None]
    for k in KS:
        assert rk.ambiguous(k, TOL, order=True).size == 0
        want_v, want_i = rk.topk(k)
        got_v, got_i = _knn(Q, L, k, metric)
        assert 0 <= got_i.min() and got_i.max() < nl
        assert all(np.unique(r).size == k for r in got_i)                         # distinct
        # the returned value is the fp64 value at the returned index, within the metric's tolerance
        key, sc = rk.K[rows, got_i], rk.S[rows, got_i]
        if metric == "euclidean":
            # d2 carries the bound; the returned distance is its fp32 root, one more rounding: 2^-24 of d, 2^-23 of its square
            err = np.maximum(np.abs(got_v.astype(np.float64) ** 2 - key) - 2.0 ** -23 * key, 0.0)
        else:
            err = np.abs(got_v.astype(np.float64) - R.reported(key, metric))
        print(f"{metric} ({nq}, {nl}) k={k}: max error / tolerance = {(err / (TOL * sc)).max():.3f}")
        assert (err <= TOL * sc).all()
        # sorted: best first
        assert (np.diff(got_v, axis=1) >= 0).all() if metric == "euclidean" else (np.diff(got_v, axis=1) <= 0).all()
        # everything that beats the k-th by more than tol is present; nothing returned loses to it by more than tol
        m = rk.margins(k, TOL)
        present = np.zeros(m.shape, dtype=bool)
        present[rows, got_i] = True
        assert not ((m < -1.0) & ~present).any()
        assert (m[rows, got_i] <= 1.0).all()
        # no ambiguous query is left, so the indices are the reference's
        assert np.array_equal(got_i, want_i), np.flatnonzero((got_i != want_i).any(1))[:5]


# ------------------------------------------------------------------------------------------ 4. skip / similar_drugs
def test_similar_drugs_skips_self():
    from madrigal_amd import ops, pipeline
    n = 300
    Q, L = _integers(33, n, seed=3)
    z = _cuda(L)
    me = np.arange(n)
    for metric, k in (("cosine", 5), ("euclidean", 20), ("dot", 32)):
        want_v, want_i = R.topk(L, L, k, metric, skip=me)
        v, i = pipeline.similar_drugs(z, k, metric=metric)
        assert i.dtype == torch.int64 and v.dtype == torch.float32 and i.shape == (n, k)
        i = i.cpu().numpy()
        assert not (i == me[:, None]).any()
        if metric != "cosine":                                                    # exact integers: the reference with the diagonal removed
            assert np.array_equal(i, want_i) and np.array_equal(v.cpu().numpy(), want_v.astype(np.float32))
        rows = [299, 0, 128, 128, 7]
        vr, ir = pipeline.similar_drugs(z, k, rows=rows, metric=metric)
        assert torch.equal(ir.cpu(), torch.from_numpy(i[rows])) and torch.equal(vr, v[rows])
    small = z[:9]
    v, i = pipeline.similar_drugs(small, 8, metric="dot")                         # k = nl - 1: every other drug
    assert sorted(i[4].tolist()) == [0, 1, 2, 3, 5, 6, 7, 8]
    with pytest.raises(ValueError):
        pipeline.similar_drugs(small, 9)                                          # k = nl with one skipped
    with pytest.raises(ValueError):
        pipeline.similar_drugs(z, 33)
    with pytest.raises(ValueError):
        ops.knn_topk(z, z, 33)
    with pytest.raises(ValueError):
        ops.knn_topk(small, small, 10)                                            # torch.topk raises here
    # cosine on real values: the fp64 reference with the diagonal removed
    Qr, Lr, _ = _reals(77, 300)
    rk = R.Ranked(Lr, Lr, "cosine", skip=me)
    ok = np.setdiff1d(me, rk.ambiguous(5, TOL, order=True))
    assert ok.size > 250
    i = pipeline.similar_drugs(_cuda(Lr), 5)[1].cpu().numpy()
    assert np.array_equal(i[ok], rk.topk(5)[1][ok]) and not (i == me[:, None]).any()


# ------------------------------------------------------------------------------------------ 5. the existing sweep
@pytest.mark.parametrize("n", [20, 257, 1000])
def test_indices_agree_with_match_counts(golden, n):
    from madrigal_amd import ops, retrieval as RT
    g = golden("pretrain_eval")
    X, Y = _cuda(g[f"n{n}_x"]), _cuda(g[f"n{n}_y"])
    counts = ops.pair_match_counts(X, Y)
    me = torch.arange(n, device="cuda")
    for k in (1, 5, 20):
        rows, cols = RT.inst_dist_topk_indices(X, Y, k)
        assert rows.dtype == cols.dtype == torch.int64 and rows.shape == cols.shape == (n, k)
        misses = 0
        for topk, cnt in ((rows, counts["cos_row"].long()), (cols, counts["cos_col"].long())):
            inside = cnt < k
            at = topk.gather(1, cnt.clamp(max=k - 1)[:, None])[:, 0]
            assert torch.equal(at[inside], me[inside])                            # index i sits at position cos[i] of row i
            assert not (topk[~inside] == me[~inside, None]).any()
            misses = misses + (~(topk == me[:, None]).any(1)).sum()
        acc = float(1 - RT.topk_fraction(misses, 2 * n))
        assert acc == RT.get_inst_dist_topk_accuracy(X, Y, k)[0]


# ------------------------------------------------------------------------------------------ 6. the classifier
@pytest.mark.parametrize("ntr,nte", [(300, 77), (1000, 257)])
def test_classifier_reproduces_reference(golden, ntr, nte):
    from madrigal_amd import retrieval as RT
    g = golden("knn")
    train, test = g[f"n{ntr}_train"].astype(np.float32), g[f"n{ntr}_test"].astype(np.float32)
    ctrain, ctest = _cuda(train), _cuda(test)
    for nc in CLASSES:
        lab, want = g[f"n{ntr}_train_labels_c{nc}"], g[f"n{ntr}_test_labels_c{nc}"]
        for metric in METRICS:
            for k in KS:
                gv, gi = _knn(test, train, k, metric)
                assert np.array_equal(np.sort(gi, 1), np.sort(R.topk(test, train, k, metric)[1], 1))           # no query is ambiguous
                for T in TS:
                    acc = RT.knn_classifier(ctrain, torch.from_numpy(lab.astype(np.int64)), ctest, torch.from_numpy(want.astype(np.int64)),
                                            metric=metric, k=k, T=T, num_classes=nc)
                    assert isinstance(acc, float) and acc == float(g[case_key(ntr, k, metric, T, nc)]), (nc, metric, k, T)
                    pred, sums = RT.knn_predict(train, lab, test, metric=metric, k=k, T=T, num_classes=nc)     # CPU input is moved
                    rp, rs, _ = R.vote(gv, gi, lab, T, nc)                         # the epilogue in fp64 on the same lists
                    assert pred.dtype == torch.uint8 and sums.shape == (nte, nc)
                    assert np.array_equal(pred.cpu().numpy(), rp)
                    got = sums.cpu().numpy()
                    if nc == 2:
                        # p1 is a sum of weights: rtol 1e-5.  p0 = (sum of all weights) - p1 is defined as a difference of two such
                        # sums, so what it inherits from them is 1e-5 of (sum + p1), not of itself.
                        np.testing.assert_allclose(got[:, 1], rs[:, 1], rtol=1e-5, atol=0)
                        assert (np.abs(got[:, 0] - rs[:, 0]) <= 1e-5 * (rs.sum(1) + rs[:, 1])).all()
                    else:
                        np.testing.assert_allclose(got, rs, rtol=1e-5, atol=0)


def test_label_columns_equal_separate_calls(golden):
    from madrigal_amd import retrieval as RT
    g = golden("knn")
    train, test = _cuda(g["n300_train"]), _cuda(g["n300_test"])
    rng = np.random.default_rng(4)
    C = 5
    lab, want = rng.integers(0, 2, (300, C)).astype(np.uint8), rng.integers(0, 2, (77, C)).astype(np.uint8)
    for metric, k, T in (("cosine", 5, 0.07), ("euclidean", 20, 1.0)):
        acc = RT.knn_classifier(train, lab, test, want, metric=metric, k=k, T=T)
        assert acc.dtype == torch.float32 and acc.shape == (C,)
        pred, sums = RT.knn_predict(train, lab, test, metric=metric, k=k, T=T)
        assert pred.shape == (77, C) and sums.shape == (77, C, 2)
        for c in range(C):
            one = RT.knn_classifier(train, lab[:, c], test, want[:, c], metric=metric, k=k, T=T)
            assert float(acc[c]) == np.float32(one)
            p1, s1 = RT.knn_predict(train, lab[:, c], test, metric=metric, k=k, T=T)
            assert torch.equal(p1, pred[:, c]) and torch.equal(s1, sums[:, c])


def test_vote_tie_goes_to_lowest_class():
    from madrigal_amd import ops
    vals = torch.zeros(2, 4, device="cuda")                                      # equal weights
    idx = torch.tensor([[0, 1, 2, 3], [3, 2, 1, 0]], dtype=torch.int32, device="cuda")
    pred, sums = ops.knn_vote(vals, idx, torch.tensor([1, 0, 1, 0], dtype=torch.uint8, device="cuda"), 1.0, 2)
    assert pred.tolist() == [0, 0] and sums.tolist() == [[2.0, 2.0], [2.0, 2.0]]
    pred, sums = ops.knn_vote(vals, idx, torch.tensor([3, 1, 3, 1], dtype=torch.uint8, device="cuda"), 0.5, 5)
    assert pred.tolist() == [1, 1] and sums.tolist() == [[0.0, 2.0, 0.0, 2.0, 0.0]] * 2
    pred, _ = ops.knn_vote(vals, idx, torch.tensor([3, 3, 3, 1], dtype=torch.uint8, device="cuda"), 0.5, 5)
    assert pred.tolist() == [3, 3]


# ------------------------------------------------------------------------------------------ 7. bad input
def test_bad_input_raises():
    Q, L = (a.copy() for a in _integers(33, 300))
    bad = L.copy()
    bad[299, 127] = np.nan
    for metric in R.METRICS:
        with pytest.raises(ValueError, match="NaN"):
            _knn(Q, bad, 5, metric)
        with pytest.raises(ValueError, match="NaN"):
            _knn(bad[200:], L, 5, metric)
    zero = L.copy()
    zero[128] = 0.0
    with pytest.raises(ValueError, match="zero-norm"):
        _knn(Q, zero, 5, "cosine")
    with pytest.raises(ValueError, match="zero-norm"):
        _knn(zero[100:140], L, 5, "cosine")
    for metric in ("dot", "euclidean"):
        want_v, want_i = R.topk(Q, zero, 5, metric)
        got_v, got_i = _knn(Q, zero, 5, metric)
        assert np.array_equal(got_i, want_i) and np.array_equal(got_v, want_v.astype(np.float32))


# ------------------------------------------------------------------------------------------ 8. determinism
def test_two_calls_are_bit_identical():
    from madrigal_amd import ops
    Q, L, _ = _reals(257, 1000)
    q, lib = _cuda(Q), _cuda(L)
    for metric in R.METRICS:
        for segments in (1, None):
            v1, i1 = ops.knn_topk(q, lib, 20, metric=metric, segments=segments)
            v2, i2 = ops.knn_topk(q, lib, 20, metric=metric, segments=segments)
            assert torch.equal(v1, v2) and torch.equal(i1, i2)
