"""fp64 numpy restatement of GeomCA as csrc/geomca.hip and retrieval.geomca build it, written from the definitions:

  d2(x, y) = |x - y|^2 in float64 (sum of squared differences: 0 for equal rows, the same from either side).
  thresholds: float32(delta * delta) and float32(epsilon * epsilon), the products formed in float64 (``threshold``).
  1. epsilon estimate: np.random.seed(seed); m = int(nR * Rdist_ratio); i1, i2 = np.random.choice(nR, m) twice; over the m x m pairs
     with i1[a] != i2[b] the positive d2 values D (ascending), M of them; pos = percentile / 100 * (M - 1), k = floor(pos);
     epsilon = a + (b - a) (pos - k), a = sqrt(D[k]), b = sqrt(D[min(k + 1, M - 1)]).
  2. sparsification with delta = gamma * epsilon: in input order, row i is kept iff no KEPT j < i has d2(i, j) < delta^2 (strict).
  3. epsilon-graph on sparseR then sparseE: edge {i, j}, i != j, iff d2 <= epsilon^2 (non-strict); label = smallest vertex of the
     component, deg_same / deg_cross = neighbours in the same / the other set.
  4. components by size descending, then smallest vertex ascending (sorted(nx.connected_components(G), key=len, reverse=True) on a
     graph whose nodes were added in index order); consistency 1 - |r - e| / (r + e); quality = cross edges / edges, 0 without edges;
     precision / recall over the components above both thresholds; network consistency from (nR', nE'), network quality from all
     edges.

Tolerance of an fp32 d2 against these: ``knn_ref.TOL * (|x| + |y|)^2`` (tests/knn_ref.py: the 128-term fp32 chain)."""
import math

import networkx as nx
import numpy as np

from knn_ref import TOL

DEFAULTS = dict(Rdist_ratio=1.0, Rdist_percentile=5, gamma=1, reduceR=True, reduceE=True, sparsify=True, n_Rsamples=None,
                n_Esamples=None, comp_consistency_threshold=0.0, comp_quality_threshold=0.0, random_seed=42)


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def d2(X, Y, block=64):
    """[nx, ny] float64 squared distances by differences."""
    X, Y = _f64(X), _f64(Y)
    out = np.empty((X.shape[0], Y.shape[0]))
    for s in range(0, X.shape[0], block):
        diff = X[s:s + block, None, :] - Y[None, :, :]
        out[s:s + block] = np.einsum("ijk,ijk->ij", diff, diff)
    return out


def d2_tol(X, Y):
    """[nx, ny]: what an fp32 d2 of the pair may be off by."""
    nx_, ny_ = np.sqrt((_f64(X) ** 2).sum(1)), np.sqrt((_f64(Y) ** 2).sum(1))
    return TOL * (nx_[:, None] + ny_[None, :]) ** 2


def threshold(v):
    """float32(v * v) as a float64 number."""
    return float(np.float32(float(v) * float(v)))


def distance_select(X, Y, ids_x, ids_y, percentile):
    """-> (zeros, M, D[k], D[k + 1], pos) over the pairs with ids_x[a] != ids_y[b]."""
    dd = d2(X, Y)[np.asarray(ids_x)[:, None] != np.asarray(ids_y)[None, :]]
    zeros = int((dd == 0).sum())
    D = np.sort(dd[dd > 0])
    M = int(D.size)
    if M == 0:
        return zeros, 0, 0.0, 0.0, 0.0
    pos = float(percentile) / 100.0 * (M - 1)
    k = int(math.floor(pos))
    return zeros, M, float(D[k]), float(D[min(k + 1, M - 1)]), pos


def epsilon_from_select(lo, hi, pos):
    a, b = math.sqrt(lo), math.sqrt(hi)
    return a + (b - a) * (pos - math.floor(pos))


def estimate_epsilon(R, ratio, percentile):
    """Draws i1, i2 from numpy's global generator (seed it first)."""
    nR = len(R)
    m = int(nR * ratio)
    i1 = np.random.choice(nR, m)
    i2 = np.random.choice(nR, m)
    R = _f64(R)
    _, M, lo, hi, pos = distance_select(R[i1], R[i2], i1, i2, percentile)
    assert M > 0
    return epsilon_from_select(lo, hi, pos)


def sparsify(X, delta):
    """The kept input rows (ascending) by the sequential rule."""
    thr = threshold(delta)
    dd = d2(X, X)
    kept = []
    for i in range(dd.shape[0]):
        if not kept or not (dd[i, kept] < thr).any():
            kept.append(i)
    return np.asarray(kept, dtype=np.int64)


def adjacency(V, epsilon):
    A = d2(V, V) <= threshold(epsilon)
    np.fill_diagonal(A, False)
    return A


def components(V, n_r, epsilon):
    """-> (label, deg_same, deg_cross, graph)."""
    A = adjacency(V, epsilon)
    n = A.shape[0]
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(zip(*np.nonzero(np.triu(A))))
    label = np.empty(n, dtype=np.int64)
    for comp in nx.connected_components(G):
        label[list(comp)] = min(comp)
    is_r = np.arange(n) < n_r
    same = is_r[:, None] == is_r[None, :]
    return label, (A & same).sum(1), (A & ~same).sum(1), G


def consistency(r, e):
    return 1 - abs(r - e) / (r + e)


def scores(G, n_r, n_e, consistency_threshold=0.0, quality_threshold=0.0):
    """-> (comp_stats, network_stats) as GeomCA.get_connected_components / log_network_stats form them."""
    comp_stats = {}
    net = {"num_R_points_in_qualitycomp": 0, "num_E_points_in_qualitycomp": 0}
    for ci, comp in enumerate(sorted(nx.connected_components(G), key=len, reverse=True)):
        sub = G.subgraph(comp)
        ridx = np.array(sorted(v for v in comp if v < n_r), dtype=np.int64)
        eidx = np.array(sorted(v for v in comp if v >= n_r), dtype=np.int64) - n_r
        edges = sub.number_of_edges()
        cross = sum(1 for u, v in sub.edges() if (u < n_r) != (v < n_r))
        c = consistency(len(ridx), len(eidx))
        q = cross / edges if edges else 0
        comp_stats[ci] = {"Ridx": ridx, "Eidx": eidx, "comp_consistency": c, "comp_quality": q, "num_edges": edges, "num_RE_edges": cross}
        if c > consistency_threshold and q > quality_threshold:
            net["num_R_points_in_qualitycomp"] += len(ridx)
            net["num_E_points_in_qualitycomp"] += len(eidx)
    edges = G.number_of_edges()
    cross = sum(1 for u, v in G.edges() if (u < n_r) != (v < n_r))
    net["precision"] = net["num_E_points_in_qualitycomp"] / n_e
    net["recall"] = net["num_R_points_in_qualitycomp"] / n_r
    net["network_consistency"] = consistency(n_r, n_e)
    net["network_quality"] = cross / edges if edges else 0
    return comp_stats, net


def geomca(R, E, **parameters):
    """-> (comp_stats, network_stats, network_params) with the keys of retrieval.geomca."""
    p = dict(DEFAULTS, **parameters)
    R, E = _f64(R), _f64(E)
    np.random.seed(p["random_seed"])
    eps = float(p["epsilon"]) if p.get("epsilon") is not None else estimate_epsilon(R, p["Rdist_ratio"], p["Rdist_percentile"])
    delta = eps * p["gamma"]

    def reduce_(X, flag, n_samples):
        if not flag:
            return np.arange(len(X))
        return sparsify(X, delta) if p["sparsify"] else np.random.choice(np.arange(len(X)), n_samples)

    ri = reduce_(R, p["reduceR"], p["n_Rsamples"])
    ei = reduce_(E, p["reduceE"], p["n_Esamples"])
    n_r, n_e = len(ri), len(ei)
    _, _, _, G = components(np.concatenate([R[ri], E[ei]]), n_r, eps)
    comp_stats, net = scores(G, n_r, n_e, p["comp_consistency_threshold"], p["comp_quality_threshold"])
    params = {"num_R_points": n_r, "num_E_points": n_e, "num_RE_points": n_r + n_e, "epsilon": eps, "gamma": p["gamma"],
              "comp_consistency_threshold": p["comp_consistency_threshold"], "comp_quality_threshold": p["comp_quality_threshold"],
              "sparseR_index": np.asarray(ri, dtype=np.int64), "sparseE_index": np.asarray(ei, dtype=np.int64)}
    return comp_stats, net, params


def comp_table(comp_stats):
    """[(|Ridx|, |Eidx|, consistency, quality)] in component order."""
    return [(len(v["Ridx"]), len(v["Eidx"]), float(v["comp_consistency"]), float(v["comp_quality"])) for _, v in sorted(comp_stats.items())]
