#!/usr/bin/env python3
"""Record tests/golden/geomca.npz from the REFERENCE's own GeomCA class.

TEST INFRASTRUCTURE ONLY: needs a checkout of the reference, scipy and networkx; no GPU.
    python scripts/gen_geomca_golden.py --ref <reference checkout> [--out tests/golden/geomca.npz]

The reference module imports gudhi, umap and matplotlib, so it is not imported: its file is parsed with ``ast`` and only the class
``GeomCA`` (madrigal/evaluate/GeomCA.py) is executed (as scripts/gen_knn_golden.py does for knn_classifier), with a stand-in
``gudhi`` namespace holding GUDHI's two documented rules in numpy -- ``subsampling.sparsify_point_set`` drops a later point whose
squared distance to a kept one is < min_squared_dist; ``RipsComplex`` keeps edges of length <= max_edge_length -- no-op
``plot_ptns`` / ``plot_dist_hist`` and a temporary ``experiment_path``.

Cases: (nR, nE, gamma).  6 centres ~ 1.2 N(0,1) in a 3-dimensional latent space, spread 0.25; E lacks one centre and is shifted by
0.05; a random orthonormal 128 x 3 embedding; coordinates rounded to a grid of 1/64 and clipped to [-2, 2], stored as float16.  On
that grid every squared distance is a multiple of 2^-12 far below 2^10, so fp32 arithmetic on it is exact.  ``Rdist_percentile`` is
chosen per case so that the interpolation position is k + 0.5 with D[k] < D[k+1] the first distinct neighbours at or above the 5 %
position that leave the margin below: epsilon then lies between two data distances, not on one.

Conditions (asserted; the seed of a case is advanced until they hold): no squared distance of any pair of R u E equals or lies
within 2^-13 of delta^2 or epsilon^2, and tests/geomca_ref.py reproduces every recorded value exactly (epsilon to 1e-12)."""
from __future__ import annotations

import argparse
import ast
import logging
import math
import os
import pickle
import sys
import tempfile
import types

import networkx as nx
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import geomca_ref as G  # noqa: E402

CASES = ((150, 140, 0.5), (150, 140, 1.0), (200, 180, 0.7))
CENTRES, GRID, MARGIN, SEED = 6, 64.0, 2.0 ** -13, 42


def _d2(X, Y):
    return G.d2(X, Y)


class _Subsampling:
    @staticmethod
    def sparsify_point_set(points, min_squared_dist):
        points = np.asarray(points, dtype=np.float64)
        dd = _d2(points, points)
        kept = []
        for i in range(len(points)):
            if not kept or not (dd[i, kept] < min_squared_dist).any():
                kept.append(i)
        return [points[i] for i in kept]


class _SimplexTree:
    def __init__(self, simplices):
        self._s = simplices

    def get_skeleton(self, dim):
        return iter(self._s)


class _RipsComplex:
    def __init__(self, points, max_edge_length):
        self.points, self.max_edge_length = np.asarray(points, dtype=np.float64), max_edge_length

    def create_simplex_tree(self, max_dimension):
        dist = np.sqrt(_d2(self.points, self.points))
        n = len(self.points)
        s = [([i], 0.0) for i in range(n)]
        s += [([i, j], float(dist[i, j])) for i in range(n) for j in range(i + 1, n) if dist[i, j] <= self.max_edge_length]
        return _SimplexTree(s)


def load_reference(ref_root: str):
    from datetime import timedelta
    from timeit import default_timer as timer

    from scipy.spatial.distance import cdist
    gudhi = types.SimpleNamespace(subsampling=_Subsampling, RipsComplex=_RipsComplex)
    ns = {"np": np, "nx": nx, "gudhi": gudhi, "cdist": cdist, "logging": logging, "pickle": pickle, "os": os, "timer": timer,
          "timedelta": timedelta}
    rel = os.path.join("madrigal", "evaluate", "GeomCA.py")
    tree = ast.parse(open(os.path.join(ref_root, rel)).read())
    defs = [node for node in tree.body if isinstance(node, ast.ClassDef) and node.name == "GeomCA"]
    assert len(defs) == 1, rel
    exec(compile(ast.Module(body=defs, type_ignores=[]), rel, "exec"), ns)
    cls = ns["GeomCA"]
    cls.plot_ptns = lambda self, *a, **k: None
    cls.plot_dist_hist = lambda self, *a, **k: None
    return cls


def draw(nR, nE, seed):
    rng = np.random.default_rng([seed, nR, nE])
    centres = 1.2 * rng.standard_normal((CENTRES, 3))
    Q, _ = np.linalg.qr(rng.standard_normal((128, 3)))
    zr = centres[rng.integers(0, CENTRES, nR)] + 0.25 * rng.standard_normal((nR, 3))
    ze = centres[rng.integers(0, CENTRES - 1, nE)] + 0.25 * rng.standard_normal((nE, 3)) + 0.05
    grid = lambda z: np.clip(np.round(z @ Q.T * GRID) / GRID, -2.0, 2.0).astype(np.float16)
    return grid(zr), grid(ze)


def percentile_for(R, E, gamma):
    """The percentile whose interpolation position is k + 0.5 between two distinct neighbours D[k] < D[k+1] of the pairs the
    reference draws after np.random.seed(SEED): the first such k at or above the 5 % position (and below the 10 % position) for
    which no squared distance of R u E lies within MARGIN of epsilon^2 or delta^2.  (The first distinct neighbours are as a rule
    adjacent grid values, 2^-12 apart, and epsilon^2 then lies within 2^-13 of both.)  None when there is no such k."""
    np.random.seed(SEED)
    n = len(R)
    i1, i2 = np.random.choice(n, n), np.random.choice(n, n)
    dd = _d2(R[i1], R[i2])
    D = np.sort(dd[dd > 0])
    V = np.concatenate([R, E])
    allv = np.unique(_d2(V, V))
    for k in range(int(math.floor(0.05 * (D.size - 1))), int(math.floor(0.10 * (D.size - 1)))):
        if D[k] == D[k + 1]:
            continue
        eps = 0.5 * (math.sqrt(D[k]) + math.sqrt(D[k + 1]))
        if all(np.abs(allv - t).min() >= MARGIN for t in ((eps * gamma) ** 2, eps ** 2)):
            return 100.0 * (k + 0.5) / (D.size - 1)
    return None


def row_indices(points, X):
    """The first input row equal to each returned point."""
    out = []
    for p in np.asarray(points):
        hit = np.flatnonzero((X == p[None, :]).all(1))
        assert hit.size >= 1
        out.append(int(hit[0]))
    return np.asarray(out, dtype=np.int64)


def clear_of_thresholds(R, E, eps, gamma):
    V = np.concatenate([R, E])
    dd = _d2(V, V)
    return all(np.abs(dd - t).min() >= MARGIN for t in ((eps * gamma) ** 2, eps ** 2))


def run_case(cls, nR, nE, gamma, seed, tmp):
    R16, E16 = draw(nR, nE, seed)
    R, E = R16.astype(np.float64), E16.astype(np.float64)
    pct = percentile_for(R, E, gamma)
    if pct is None:
        return None
    params = {"experiment_path": tmp, "experiment_filename_prefix": "", "subfolder": "golden", "Rdist_ratio": 1.0, "Rdist_percentile": pct,
              "gamma": gamma, "reduceR": True, "reduceE": True, "sparsify": True, "n_Rsamples": None, "n_Esamples": None,
              "log_reduced": False, "comp_consistency_threshold": 0.0, "comp_quality_threshold": 0.0, "random_seed": SEED}
    obj = cls(R, E, params, load_existing=False, subfolder="golden")
    comp_stats, net, netp = obj.get_connected_components()
    eps = float(netp["epsilon"])
    if not clear_of_thresholds(R, E, eps, gamma):
        return None
    ri, ei = row_indices(obj.sparseR, R), row_indices(obj.sparseE, E)
    table = np.array([(len(v["Ridx"]), len(v["Eidx"]), v["comp_consistency"], v["comp_quality"]) for _, v in sorted(comp_stats.items())],
                     dtype=np.float64)
    scores = np.array([net["precision"], net["recall"], net["network_consistency"], net["network_quality"]], dtype=np.float64)
    edges = obj.RE_network.number_of_edges()
    # the restatement reproduces every recorded value
    mine = G.geomca(R, E, Rdist_percentile=pct, gamma=gamma, random_seed=SEED)
    assert abs(mine[2]["epsilon"] - eps) <= 1e-12 * eps, (mine[2]["epsilon"], eps)
    assert mine[2]["sparseR_index"].tolist() == ri.tolist() and mine[2]["sparseE_index"].tolist() == ei.tolist()
    assert np.array_equal(np.array(G.comp_table(mine[0])), table)
    assert [mine[1][k] for k in ("precision", "recall", "network_consistency", "network_quality")] == scores.tolist()
    assert sum(v["num_edges"] for v in mine[0].values()) == edges
    return {"R": R16, "E": E16, "gamma": np.float64(gamma), "percentile": np.float64(pct), "epsilon": np.float64(eps), "sparseR_index": ri,
            "sparseE_index": ei, "components": table, "scores": scores, "edges": np.int64(edges)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "geomca.npz"))
    a = ap.parse_args()
    cls = load_reference(a.ref)
    out = {"cases": np.array(CASES, dtype=np.float64)}
    with tempfile.TemporaryDirectory() as tmp:
        for ci, (nR, nE, gamma) in enumerate(CASES):
            for seed in range(200):
                rec = run_case(cls, nR, nE, gamma, seed, tmp)
                if rec is not None:
                    break
            else:
                raise RuntimeError(f"case {ci}: no seed below 200 keeps every squared distance clear of the thresholds")
            out.update({f"c{ci}_{k}": v for k, v in rec.items()})
            out[f"c{ci}_seed"] = np.int64(seed)
            print(f"case {ci}: nR {nR} nE {nE} gamma {gamma} seed {seed} percentile {float(rec['percentile']):.6f} epsilon "
                  f"{float(rec['epsilon']):.6f} kept {rec['sparseR_index'].size} / {rec['sparseE_index'].size} edges {int(rec['edges'])} "
                  f"components {rec['components'].shape[0]} scores {rec['scores'].tolist()}")
        logging.shutdown()
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
