"""On-device GeomCA (csrc/geomca.hip, ops.geomca_*, retrieval.geomca, evaluate.get_alignment_metrics / evaluate_final_embeds) against
the fp64 restatement tests/geomca_ref.py and the values recorded from the reference's own class (tests/golden/geomca.npz).

Exact comparisons run on inputs whose fp32 arithmetic is exact (integers, dyadic grids) or, for real-valued data, with thresholds
placed in gaps of the fp64 squared distances at least four tolerances wide (asserted on the CPU first)."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geomca_ref as G                                           # noqa: E402
from test_geomca_cpu import SCORE_KEYS, golden_case, line        # noqa: E402

pytestmark = pytest.mark.gpu

SEGMENTS = (1, 2, 3, None)


def _cuda(x, dtype=torch.float32):
    return torch.from_numpy(np.array(x, order="C")).to(dtype).cuda()              # a copy: cached inputs are read-only


def _components(V, n_r, eps, segments=None):
    from madrigal_amd import ops
    label, same, cross, sweeps = ops.geomca_components(_cuda(V), n_r, eps, segments=segments)
    assert label.dtype == same.dtype == cross.dtype == torch.int32 and label.shape == same.shape == cross.shape == (len(V),)
    return label.cpu().numpy(), same.cpu().numpy(), cross.cpu().numpy(), sweeps


def _sparsify(X, delta, **kw):
    from madrigal_amd import ops
    kept = ops.geomca_sparsify(_cuda(X), delta, **kw)
    assert kept.dtype == torch.int64 and kept.dim() == 1
    return kept.cpu().numpy()


def _assert_components(V, n_r, eps, segments=None):
    want = G.components(V, n_r, eps)[:3]
    got = _components(V, n_r, eps, segments)
    for name, w, g_ in zip(("label", "deg_same", "deg_cross"), want, got):
        assert np.array_equal(w, g_), (name, len(V), n_r, eps, segments, np.flatnonzero(w != g_)[:8])
    return got


@functools.lru_cache(maxsize=None)
def _integers(n, seed=0):
    """Entries in {-2..2}: every squared distance is an exact fp32 integer; a third of the rows are copies of other rows."""
    rng = np.random.default_rng([seed, n])
    X = rng.integers(-2, 3, (n, 128)).astype(np.float32)
    dup = rng.integers(0, n, max(n // 3, 1))
    X[dup] = X[rng.integers(0, n, dup.size)]
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _lattice(n, seed=0):
    """Integer points of a 3-dimensional lattice in [-6, 6]^3 (the other coordinates are 0), with repeats: squared distances are
    small integers, most of them attained many times."""
    rng = np.random.default_rng([seed, n, 3])
    X = np.zeros((n, 128), dtype=np.float32)
    X[:, [0, 50, 127]] = rng.integers(-6, 7, (n, 3))
    X.setflags(write=False)
    return X


# ------------------------------------------------------------------------------------------ 1. the d2 identities
@pytest.mark.parametrize("n", [1, 2, 31, 33, 127, 128, 129, 257])
def test_components_on_integers_with_duplicates_equal_the_restatement(n):
    X = _integers(n)
    dd = G.d2(X, X)
    pos = np.sort(dd[dd > 0])
    eps2 = [0.0] + ([float(pos[pos.size // 10]), float(pos[pos.size // 2])] if pos.size else [])       # attained values
    for n_r in sorted({0, 1, n // 2 + (1 if n > 2 else 0), n} & set(range(n + 1))):
        for e2 in eps2:
            eps = math.sqrt(e2)
            assert G.threshold(eps) == e2                                        # float32(eps * eps) IS the attained value
            label, same, cross, _ = _assert_components(X, n_r, eps)
            is_r = np.arange(n) < n_r
            assert same[is_r].sum() % 2 == 0 and same[~is_r].sum() % 2 == 0 and cross[is_r].sum() == cross[~is_r].sum()
            if e2 == 0.0:                                                        # bitwise-equal rows are at d2 == 0 exactly
                first = np.array([np.flatnonzero((X == X[i]).all(1))[0] for i in range(n)])
                assert np.array_equal(label, first)
                assert np.array_equal(same + cross, np.array([((X == X[i]).all(1)).sum() - 1 for i in range(n)]))


def test_nan_and_inf_raise_and_runs_repeat():
    from madrigal_amd import ops
    X = _integers(129).copy()
    for bad in (np.nan, np.inf):
        Y = X.copy()
        Y[77, 100] = bad
        for fn in (lambda t: ops.geomca_sparsify(t, 1.0), lambda t: ops.geomca_components(t, 5, 1.0), ops.geomca_prep,
                   lambda t: ops.geomca_distance_select(t, t, torch.arange(129).cuda(), torch.arange(129).cuda(), 5.0)):
            with pytest.raises(ValueError, match="NaN"):
                fn(_cuda(Y))
    with pytest.raises(ValueError):
        ops.geomca_sparsify(_cuda(X), 1.0, chunk=100)
    with pytest.raises(ValueError):
        ops.geomca_components(_cuda(X), 130, 1.0)
    with pytest.raises(ValueError):
        ops.geomca_components(_cuda(X), 5, float("nan"))
    with pytest.raises(ValueError):
        ops.geomca_sparsify(_cuda(X)[:, :64], 1.0)
    a, b = _components(X, 60, 20.0), _components(X, 60, 20.0)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    assert np.array_equal(_sparsify(X, 20.0), _sparsify(X, 20.0))


# ------------------------------------------------------------------------------------------ 2. sparsification
@pytest.mark.parametrize("chunk", [None, 128])
def test_sparsify_exact_kept_lists_at_the_chunk_edges(chunk):
    from madrigal_amd import ops
    C = chunk or ops.geomca_default_chunk()
    for n in (1, 127, 128, 129, C - 1, C, C + 1, 2 * C + 77):
        X = _lattice(n)
        for delta2 in (9.0, 2.0):                                                # attained values: d2 == delta^2 must not drop
            delta = math.sqrt(delta2)
            assert G.threshold(delta) == delta2
            want = G.sparsify(X, delta)
            got = _sparsify(X, delta, chunk=chunk)
            assert np.array_equal(want, got), (n, chunk, delta2, want[:10], got[:10])
            assert 1 <= got.size < n or n == 1


def test_sparsify_is_the_same_for_every_chunk_and_segment_count():
    from madrigal_amd import ops
    n = 2 * ops.geomca_default_chunk() + 77
    X = _lattice(n, seed=1)
    base = _sparsify(X, 3.0)
    assert np.array_equal(base, G.sparsify(X, 3.0))
    for chunk in (128, None):
        for seg in SEGMENTS:
            assert np.array_equal(base, _sparsify(X, 3.0, chunk=chunk, segments=seg)), (chunk, seg)


@pytest.mark.parametrize("chunk", [None, 128])
def test_sparsify_cascade_trap_across_chunk_edges(chunk):
    """A line at spacing 0.6 delta (0.75 against delta = 1.25, dyadic: fp32 exact), longer than two chunks: every point is within
    delta of both neighbours, so the alternate points are kept and each dropped point lies within delta of its successor.  A
    resolver that let a DROPPED point drop others would keep one in three or fewer; the chunk edges fall on kept and dropped points."""
    from madrigal_amd import ops
    C = chunk or ops.geomca_default_chunk()
    n = 2 * C + 77
    X = line(0.75 * (np.arange(n) - n // 2))
    want = np.arange(0, n, 2)
    assert np.array_equal(G.sparsify(X, 1.25), want)
    for seg in (None, 1, 3):
        assert np.array_equal(_sparsify(X, 1.25, chunk=chunk, segments=seg), want), seg
    # the same points visited from the far end, and with a kept point exactly at distance delta (spacing 1.25: nothing is dropped)
    assert np.array_equal(_sparsify(X[::-1].copy(), 1.25, chunk=chunk), want)
    Y = line(1.25 * (np.arange(n) - n // 2))
    assert np.array_equal(_sparsify(Y, 1.25, chunk=chunk), np.arange(n))


@pytest.mark.parametrize("chunk", [None, 128])
def test_sparsify_all_equal_and_all_apart(chunk):
    from madrigal_amd import ops
    n = 2 * (chunk or ops.geomca_default_chunk()) + 77
    same = np.tile(_integers(1, seed=3), (n, 1))
    assert _sparsify(same, 0.5, chunk=chunk).tolist() == [0]
    assert _sparsify(same, 0.0, chunk=chunk).tolist() == list(range(n))           # d2 == 0 is not < 0
    apart = line(2.0 * (np.arange(n) - n // 2))
    assert np.array_equal(_sparsify(apart, 1.0, chunk=chunk), np.arange(n))
    assert np.array_equal(_sparsify(apart, 2.0, chunk=chunk), np.arange(n))       # d2 == delta^2 = 4 does not drop


# ------------------------------------------------------------------------------------------ 3. components
def test_shuffled_path_graph_is_one_component():
    n = 1000
    rng = np.random.default_rng(5)
    perm = rng.permutation(n)
    V = line((perm - n // 2).astype(np.float32))                                 # vertex v sits at position perm[v] of the path
    for seg in SEGMENTS:
        label, same, cross, sweeps = _assert_components(V, 500, 1.0, seg)
        assert (label == 0).all() and (same + cross).sum() == 2 * (n - 1)
        assert 2 <= sweeps <= 2 * math.ceil(math.log2(n)) + 2, sweeps            # hooking + jumping, not the diameter
    print("path graph of 1000 shuffled vertices: link sweeps", sweeps)


def test_interleaved_sets_isolated_vertices_and_a_clique():
    # R and E interleaved on a line in groups, far-away isolated vertices of both sets, and a clique of equal-distance points
    coords_r = [0, 1, 2, 10, 11, 50, 100, 101, 102, 103]
    coords_e = [0.5, 1.5, 10.5, 30, 70, 100.5, 101.5, 102.5]
    V = line(coords_r + coords_e)
    for seg in SEGMENTS:
        label, same, cross, _ = _assert_components(V, len(coords_r), 0.5, seg)
        assert (same == 0).all() and cross[5] == 0 and cross[len(coords_r) + 3] == 0         # isolated: 50 (R), 30 and 70 (E)
        _assert_components(V, len(coords_r), 1.0, seg)
    n = 150
    Q = np.zeros((n, 128), dtype=np.float32)
    Q[np.arange(n) % n, np.arange(n) % 128] = 1.0                                # unit vectors, repeated past 128: d2 in {0, 2}
    for seg in SEGMENTS:
        label, same, cross, sweeps = _assert_components(Q, 70, math.sqrt(2.0), seg)
        assert (label == 0).all() and (same + cross == n - 1).all() and sweeps == 2
    label, same, cross, _ = _assert_components(Q, 70, 1.0)                       # below sqrt(2): only the repeats are linked
    assert (same + cross == (np.arange(n) % 128 < n - 128)).all()


def test_clustered_graph_over_many_blocks_matches_for_every_segment_count():
    X = _lattice(700, seed=2)
    base = _assert_components(X, 333, 2.0)
    for seg in (1, 2, 3):
        got = _components(X, 333, 2.0, seg)
        assert all(np.array_equal(a, b) for a, b in zip(base[:3], got[:3])) and got[3] == base[3]


# ------------------------------------------------------------------------------------------ 4. distance select
def _select(X, i1, i2, pct, segments=None):
    from madrigal_amd import ops
    x, t1, t2 = _cuda(X), _cuda(i1, torch.int64), _cuda(i2, torch.int64)
    return ops.geomca_distance_select(x.index_select(0, t1), x.index_select(0, t2), t1, t2, pct, segments=segments)


@pytest.mark.parametrize("m", [33, 150, 400])
def test_distance_select_on_grid_data_equals_numpy(golden, m):
    R = golden_case(golden("geomca"), 0)[0].copy()
    R[[5, 17, 60]] = R[[100, 100, 3]]                                            # duplicated rows: counted in ``zeros``
    rng = np.random.default_rng([m, 9])
    i1, i2 = rng.integers(0, len(R), m), rng.integers(0, len(R), m)             # repeated indices: i1[a] == i2[b] is left out
    assert (i1[:, None] == i2[None, :]).any()
    for pct in (0, 5, 50, 100):
        want = G.distance_select(R[i1], R[i2], i1, i2, pct)
        assert want[0] > 0 and want[1] > 0
        for seg in ((None, 1, 3) if pct == 5 else (None,)):
            got = _select(R, i1, i2, pct, seg)
            assert got == want, (m, pct, seg, got, want)
        dd = G.d2(R[i1], R[i2])[i1[:, None] != i2[None, :]]
        dist = np.sqrt(dd[dd > 0])
        assert abs(G.epsilon_from_select(*want[2:]) - np.percentile(dist, pct)) <= 1e-12 * dist.max()
    assert got[2] == got[3] == float(dd.max())                                   # percentile 100: k + 1 clamps to M - 1


def test_distance_select_on_float_data_is_within_tolerance():
    rng = np.random.default_rng(21)
    X = (rng.standard_normal((200, 128)) * rng.uniform(0.5, 2.0, (200, 1))).astype(np.float32)
    i1, i2 = rng.integers(0, 200, 180), rng.integers(0, 200, 180)
    tol = G.d2_tol(X[i1], X[i2]).max()
    for pct in (0, 5, 37.5, 100):
        want = G.distance_select(X[i1], X[i2], i1, i2, pct)
        got = _select(X, i1, i2, pct)
        assert got[:2] == want[:2] and got[4] == want[4]
        # an order statistic moves by at most the largest change of any one value
        assert abs(got[2] - want[2]) <= tol and abs(got[3] - want[3]) <= tol and got[2] <= got[3]


def test_distance_select_without_positive_distances():
    X = np.tile(_integers(1, seed=4), (40, 1))
    ids = np.arange(40)
    assert _select(X, ids, ids, 5.0) == (40 * 39, 0, 0.0, 0.0, 0.0)
    from madrigal_amd import retrieval
    with pytest.raises(ValueError, match="epsilon"):
        retrieval.geomca(_cuda(X), _cuda(X))


# ------------------------------------------------------------------------------------------ 5. end to end on the recorded cases
@pytest.mark.parametrize("ci", [0, 1, 2])
def test_geomca_reproduces_the_recorded_reference(golden, ci):
    from madrigal_amd import retrieval
    R, E, gamma, pct, rec = golden_case(golden("geomca"), ci)
    comp, net, par = retrieval.geomca(_cuda(R), _cuda(E), Rdist_percentile=pct, gamma=gamma)
    eps = float(rec["epsilon"])
    assert abs(par["epsilon"] - eps) <= 1e-12 * eps
    assert par["sparseR_index"].tolist() == rec["sparseR_index"].tolist()
    assert par["sparseE_index"].tolist() == rec["sparseE_index"].tolist()
    assert np.array_equal(np.array(G.comp_table(comp)), rec["components"])
    assert [net[k] for k in SCORE_KEYS] == rec["scores"].tolist()
    assert sum(v["num_edges"] for v in comp.values()) == int(rec["edges"])
    assert (par["num_R_points"], par["num_E_points"], par["num_RE_points"]) == (len(rec["sparseR_index"]), len(rec["sparseE_index"]),
                                                                                  len(rec["sparseR_index"]) + len(rec["sparseE_index"]))
    assert set(par) == {"num_R_points", "num_E_points", "num_RE_points", "epsilon", "gamma", "comp_consistency_threshold",
                        "comp_quality_threshold", "sparseR_index", "sparseE_index"}
    assert set(net) == {"num_R_points_in_qualitycomp", "num_E_points_in_qualitycomp", *SCORE_KEYS}
    assert set(comp[0]) == {"Ridx", "Eidx", "comp_consistency", "comp_quality", "num_edges", "num_RE_edges"}


def test_geomca_options_follow_the_restatement(golden):
    """reduceX = False, the sampling route (numpy's global generator, R then E after the estimate's two draws), thresholds."""
    from madrigal_amd import retrieval
    R, E, gamma, pct, rec = golden_case(golden("geomca"), 0)
    for kw in (dict(reduceR=False), dict(reduceE=False, comp_consistency_threshold=0.5), dict(sparsify=False, n_Rsamples=60, n_Esamples=50),
               dict(epsilon=float(rec["epsilon"]), comp_quality_threshold=0.4), dict(Rdist_ratio=0.5, random_seed=7, epsilon=None)):
        kw = dict(dict(Rdist_percentile=pct, gamma=gamma), **kw)
        if kw.get("Rdist_ratio") == 0.5:                                         # another draw: epsilon may sit on a tie, so pin it
            kw["epsilon"] = G.geomca(R, E, **kw)[2]["epsilon"]
        want, got = G.geomca(R, E, **kw), retrieval.geomca(_cuda(R), _cuda(E), **kw)
        assert got[2]["sparseR_index"].tolist() == want[2]["sparseR_index"].tolist(), kw
        assert got[2]["sparseE_index"].tolist() == want[2]["sparseE_index"].tolist(), kw
        assert G.comp_table(got[0]) == G.comp_table(want[0]) and got[1] == want[1], kw
        for c in want[0]:
            assert all(np.array_equal(got[0][c][k], want[0][c][k]) for k in ("Ridx", "Eidx"))
            assert (got[0][c]["num_edges"], got[0][c]["num_RE_edges"]) == (want[0][c]["num_edges"], want[0][c]["num_RE_edges"])
    with pytest.raises(ValueError, match="unknown"):
        retrieval.geomca(_cuda(R), _cuda(E), gama=1)
    with pytest.raises(ValueError, match="empty"):
        retrieval.geomca(_cuda(R), _cuda(E), sparsify=False, n_Rsamples=0, n_Esamples=5, epsilon=0.4)


# ------------------------------------------------------------------------------------------ 6. real-valued data
@functools.lru_cache(maxsize=None)
def _float_case(seed):
    """Clustered fp32 points off any grid (R 120, E 100) and (epsilon, delta) whose squares sit in the middle of gaps of the fp64
    squared distances of R u E at least four tolerances wide; None when this seed has no such gaps near the wanted quantiles."""
    rng = np.random.default_rng([seed, 77])
    centres = 0.6 * rng.standard_normal((5, 3))
    Q, _ = np.linalg.qr(rng.standard_normal((128, 3)))
    R = ((centres[rng.integers(0, 5, 120)] + 0.25 * rng.standard_normal((120, 3))) @ Q.T).astype(np.float32)
    E = ((centres[rng.integers(0, 4, 100)] + 0.25 * rng.standard_normal((100, 3)) + 0.05) @ Q.T).astype(np.float32)
    V = np.concatenate([R, E])
    tol = G.d2_tol(V, V)                                                          # per pair
    dd = G.d2(V, V)
    vals = np.unique(dd)
    gaps = np.diff(vals)

    def mid_gap(target):
        start = int(np.searchsorted(vals, target))
        for i in range(start, min(start + 3000, gaps.size)):
            mid = 0.5 * (vals[i] + vals[i + 1])
            if gaps[i] >= 4 * tol.min() and (np.abs(dd - mid) >= 2 * tol).all():  # every pair's own gap is 4 tolerances wide
                return mid
        return None
    pos = vals[vals > 0]
    e2 = mid_gap(float(np.quantile(pos, 0.04)))
    d2_ = None if e2 is None else mid_gap(0.36 * e2)
    if e2 is None or d2_ is None or d2_ >= e2:
        return None
    return R, E, math.sqrt(e2), math.sqrt(d2_), tol


def test_float_data_with_thresholds_in_gaps_equals_the_restatement():
    from madrigal_amd import retrieval
    done = 0
    for seed in range(12):
        case = _float_case(seed)
        if case is None:
            continue
        R, E, eps, delta, tol = case
        V = np.concatenate([R, E])
        dd = G.d2(V, V)
        for thr in (G.threshold(eps), G.threshold(delta)):                        # asserted before anything is compared
            assert (np.abs(dd - thr) >= 2 * tol * (1 - 1e-3)).all()
        gamma = delta / eps
        assert G.threshold(eps * gamma) == G.threshold(delta)
        want, got = G.geomca(R, E, epsilon=eps, gamma=gamma), retrieval.geomca(_cuda(R), _cuda(E), epsilon=eps, gamma=gamma)
        assert got[2]["sparseR_index"].tolist() == want[2]["sparseR_index"].tolist()
        assert got[2]["sparseE_index"].tolist() == want[2]["sparseE_index"].tolist()
        assert 10 < want[2]["num_R_points"] < 120 and want[2]["num_E_points"] < 100
        assert G.comp_table(got[0]) == G.comp_table(want[0]) and got[1] == want[1]
        n_r = want[2]["num_R_points"]
        Vs = np.concatenate([R[want[2]["sparseR_index"]], E[want[2]["sparseE_index"]]])
        _assert_components(Vs, n_r, eps)
        done += 1
        if done == 2:
            break
    assert done == 2


# ------------------------------------------------------------------------------------------ 7. the evaluate.py mirrors
class _Wandb:
    def __init__(self):
        self.calls = []

    def log(self, d, step=None):
        self.calls.append((dict(d), step))


class _Logger:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


def _outputs(X, drugs, cuda):
    t = torch.from_numpy(X)
    return {"embeds": t.cuda() if cuda else t, "drugs": np.asarray(drugs)}


def test_get_alignment_metrics_logs_geomca_of_the_shared_drugs(golden, tmp_path):
    from madrigal_amd import evaluate, retrieval
    R, E, gamma, pct, _ = golden_case(golden("geomca"), 0)
    rng = np.random.default_rng(3)
    d1 = rng.permutation(400)[:len(R)]                                           # drug ids in no order, partly shared
    d2 = np.concatenate([rng.permutation(d1)[:100], 1000 + np.arange(len(E) - 100)])
    d2 = d2[rng.permutation(len(d2))]
    shared = np.intersect1d(d1, d2)
    assert shared.size == 100 and (np.diff(shared) > 0).all()
    rows1 = np.array([np.flatnonzero(d1 == d)[0] for d in shared])
    rows2 = np.array([np.flatnonzero(d2 == d)[0] for d in shared])
    params = dict(Rdist_percentile=pct, gamma=gamma)
    want = retrieval.geomca(_cuda(R[rows1]), _cuda(E[rows2]), **params)
    for cuda in (False, True):
        wb, lg = _Wandb(), _Logger()
        got = evaluate.get_alignment_metrics("val str v kg", _outputs(R, d1, cuda), _outputs(E, d2, cuda), str(tmp_path), wb, lg, 7,
                                             parameters=params)
        assert len(wb.calls) == 1 and wb.calls[0][1] == 7
        logged = wb.calls[0][0]
        assert list(logged) == ["val str v kg GeomCA precision", "val str v kg GeomCA recall", "val str v kg GeomCA network consistency",
                                "val str v kg GeomCA network quality", "val str v kg GeomCA sample size"]
        assert [logged[k] for k in list(logged)[:4]] == [want[1][k] for k in SCORE_KEYS] and logged["val str v kg GeomCA sample size"] == 100
        assert got[1] == want[1] and got[2]["sparseR_index"].tolist() == want[2]["sparseR_index"].tolist()
        assert len(lg.lines) == 1 and "val str v kg precision" in lg.lines[0] and "sample size: 100" in lg.lines[0]
    assert list(tmp_path.iterdir()) == []                                        # save_dir is accepted and nothing is written
    with pytest.raises(ValueError, match="share"):
        evaluate.get_alignment_metrics("x", _outputs(R, d1, False), _outputs(E, 5000 + np.arange(len(E)), False), None, _Wandb(), None, 0)


def test_evaluate_final_embeds_walks_every_pair_of_both_splits(golden, tmp_path):
    from madrigal_amd import evaluate, retrieval
    g = golden("geomca")
    R, E = golden_case(g, 0)[:2]
    X2 = golden_case(g, 2)[0]
    ids = np.arange(130)
    train = {"0": _outputs(R[:130], ids, False), "1": _outputs(E[:130], ids[::-1].copy(), True), "3": _outputs(X2[:130], ids, False)}
    val = {"0": _outputs(R[20:140], ids[:120], True), "2": _outputs(E[10:130], ids[:120], False)}
    wb = _Wandb()
    assert evaluate.evaluate_final_embeds(train, val, str(tmp_path), wb, None, 3) is None
    names = [f"train {a} v {b}" for a, b in (("str", "kg"), ("str", evaluate.NUMBER2MODALITY["3"]), ("kg", evaluate.NUMBER2MODALITY["3"]))]
    names.append(f"val str v {evaluate.NUMBER2MODALITY['2']}")
    assert [sorted(c[0])[0].split(" GeomCA ")[0] for c in wb.calls] == names and all(c[1] == 3 for c in wb.calls)
    assert all(c[0][f"{nm} GeomCA sample size"] == (130 if nm.startswith("train") else 120) for c, nm in zip(wb.calls, names))
    want = retrieval.geomca(_cuda(R[:130]), _cuda(E[:130][::-1].copy()))[1]       # drug i is row i of '0' and row 129 - i of '1'
    assert [wb.calls[0][0][f"{names[0]} GeomCA {k}"] for k in ("precision", "recall", "network consistency", "network quality")] == \
        [want[k] for k in SCORE_KEYS]
    assert list(tmp_path.iterdir()) == []
