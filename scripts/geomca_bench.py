#!/usr/bin/env python3
"""Time on-device GeomCA (csrc/geomca.hip, retrieval.geomca) per stage and end to end, beside what was possible before it: dense
torch distance blocks + thresholding on the GPU, with the sequential parts (the greedy sparsification, the union of components) on
the host.  Prints one JSON line (recorded as profiles/geomca_bench.json).

    python scripts/geomca_bench.py [--rounds 3] [--shapes 4096,16384,100352] [--dense-up-to 16384] [--out profiles/geomca_bench.json]

Inputs per shape n (R and E of n rows each, D = 128): 256 centres in an 8-dimensional latent space under a random orthonormal
embedding, spread 0.25; E lacks a tenth of the centres and is shifted by 0.05.  Parameters: the defaults of get_alignment_metrics
(Rdist_ratio 1, percentile 5, gamma 1, sparsify).  Stages, each timed with a host clock around calls that end in a device
synchronise, median [min, max] over the rounds, the two routes alternating round by round:
  estimate     retrieval.geomca_epsilon: the two index draws, two gathers, three digit sweeps over the n x n pairs;
  sparsify_R/E ops.geomca_sparsify at delta = epsilon;
  components   ops.geomca_components on the kept rows of both sets;
  end_to_end   retrieval.geomca (the stages, the host scoring and the transfers).
Dense route (shapes up to --dense-up-to; its [n,n] blocks do not fit beyond): torch.cdist (by differences) of the drawn rows, ``> 0`` and a sort for
the percentile; ``cdist < delta`` to the host as a bool matrix and the greedy walk there (one vectorised OR per kept row);
``cdist <= epsilon`` on the kept rows, ``nonzero`` to the host and scipy's connected_components.  The two routes' kept rows and
component counts are compared once; they may differ where a distance lies within fp32 rounding of a threshold (cdist forms
distances, not the Gram chain).  Link sweeps per call are recorded, also for a shuffled path graph of 4096 vertices."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from madrigal_amd import ops, retrieval  # noqa: E402

PARAMS = retrieval.GEOMCA_DEFAULTS


def make_inputs(n, seed):
    rng = np.random.default_rng([seed, n])
    centres = 1.2 * rng.standard_normal((256, 8))
    Q, _ = np.linalg.qr(rng.standard_normal((128, 8)))
    zr = centres[rng.integers(0, 256, n)] + 0.25 * rng.standard_normal((n, 8))
    ze = centres[rng.integers(0, 230, n)] + 0.25 * rng.standard_normal((n, 8)) + 0.05
    return (torch.from_numpy((z @ Q.T).astype(np.float32)).cuda() for z in (zr, ze))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


# ------------------------------------------------------------------------------------------ the dense route
def cdist(x, y):
    """Distances by differences: the default matmul form leaves equal rows at small positive distances, which then pass ``> 0``."""
    rows = max(1, (1 << 22) // max(int(y.shape[0]), 1))                        # that kernel launches one block per entry
    return torch.cat([torch.cdist(x[r:r + rows], y, compute_mode="donot_use_mm_for_euclid_dist") for r in range(0, x.shape[0], rows)])


def dense_epsilon(R, ratio, percentile):
    n = R.shape[0]
    m = int(n * ratio)
    i1 = torch.from_numpy(np.random.choice(n, m)).to(R.device)
    i2 = torch.from_numpy(np.random.choice(n, m)).to(R.device)
    d = cdist(R[i1], R[i2]).flatten()
    d = d[d > 0].sort()[0]
    pos = percentile / 100.0 * (d.numel() - 1)
    k = int(np.floor(pos))
    a, b = float(d[k]), float(d[min(k + 1, d.numel() - 1)])
    return a + (b - a) * (pos - k)


def dense_sparsify(X, delta, block=4096):
    n = X.shape[0]
    near = np.empty((n, n), dtype=bool)
    for r0 in range(0, n, block):
        near[r0:r0 + block] = (cdist(X[r0:r0 + block], X) < delta).cpu().numpy()
    dropped = np.zeros(n, dtype=bool)
    kept = []
    for i in range(n):
        if not dropped[i]:
            kept.append(i)
            dropped |= near[i]
    return torch.tensor(kept, dtype=torch.int64, device=X.device)


def dense_components(V, epsilon):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n = V.shape[0]
    ij = (cdist(V, V) <= epsilon).nonzero().cpu().numpy()
    ij = ij[ij[:, 0] != ij[:, 1]]
    ncomp, label = connected_components(coo_matrix((np.ones(len(ij), dtype=np.int8), (ij[:, 0], ij[:, 1])), shape=(n, n)), directed=False)
    return ncomp, label, len(ij) // 2


def dense_geomca(R, E):
    np.random.seed(PARAMS["random_seed"])
    eps = dense_epsilon(R, PARAMS["Rdist_ratio"], PARAMS["Rdist_percentile"])
    ri, ei = dense_sparsify(R, eps * PARAMS["gamma"]), dense_sparsify(E, eps * PARAMS["gamma"])
    return eps, ri, ei, dense_components(torch.cat([R[ri], E[ei]]), eps)


# ------------------------------------------------------------------------------------------ one shape
def stats(ts):
    return {"ms": round(float(np.median(ts)), 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)], "rounds": len(ts)}


def bench_shape(n, rounds, dense):
    R, E = make_inputs(n, 0)

    def estimate():
        np.random.seed(PARAMS["random_seed"])
        return retrieval.geomca_epsilon(R, PARAMS["Rdist_ratio"], PARAMS["Rdist_percentile"])
    eps = estimate()
    delta = eps * PARAMS["gamma"]
    ri, ei = ops.geomca_sparsify(R, delta), ops.geomca_sparsify(E, delta)
    V = torch.cat([R.index_select(0, ri), E.index_select(0, ei)])
    label, _, _, sweeps = ops.geomca_components(V, int(ri.numel()), eps)
    res = {"n_R": n, "n_E": n, "epsilon": eps, "kept_R": int(ri.numel()), "kept_E": int(ei.numel()), "link_sweeps": sweeps,
           "component_count": int(label.unique().numel()), "sparsify_chunk": ops.geomca_default_chunk()}
    device = {"estimate": estimate, "sparsify_R": lambda: ops.geomca_sparsify(R, delta), "sparsify_E": lambda: ops.geomca_sparsify(E, delta),
              "components": lambda: ops.geomca_components(V, int(ri.numel()), eps), "end_to_end": lambda: retrieval.geomca(R, E)}
    variants = {"device_" + k: fn for k, fn in device.items()}
    # a quarter of delta keeps many more rows: the sparsifier's cost grows with (rows x kept rows)
    res["kept_R_quarter_delta"] = int(ops.geomca_sparsify(R, delta / 4).numel())
    variants["device_sparsify_R_quarter_delta"] = lambda: ops.geomca_sparsify(R, delta / 4)
    if dense:
        def d_estimate():
            np.random.seed(PARAMS["random_seed"])
            return dense_epsilon(R, PARAMS["Rdist_ratio"], PARAMS["Rdist_percentile"])
        d_eps, d_ri, d_ei, (d_ncomp, _, d_edges) = dense_geomca(R, E)
        res["dense_epsilon"], res["dense_kept_R"], res["dense_kept_E"], res["dense_component_count"] = d_eps, int(d_ri.numel()), int(d_ei.numel()), int(d_ncomp)
        res["kept_R_equal"] = bool(d_ri.numel() == ri.numel() and bool((d_ri == ri).all()))
        res["kept_E_equal"] = bool(d_ei.numel() == ei.numel() and bool((d_ei == ei).all()))
        variants.update({"dense_estimate": d_estimate, "dense_sparsify_R": lambda: dense_sparsify(R, delta),
                         "dense_sparsify_E": lambda: dense_sparsify(E, delta), "dense_components": lambda: dense_components(V, eps),
                         "dense_end_to_end": lambda: dense_geomca(R, E)})
    times = {v: [] for v in variants}
    for fn in variants.values():                     # warm-up
        fn()
    for _ in range(rounds):
        for v, fn in variants.items():
            times[v].append(timed(fn)[0])
    res.update({v: stats(ts) for v, ts in times.items()})
    if dense:
        for k in device:
            res[f"dense_over_device_{k}"] = round(res["dense_" + k]["ms"] / res["device_" + k]["ms"], 3)
    del R, E, V
    torch.cuda.empty_cache()
    return res


def path_graph_sweeps(n=4096):
    perm = np.random.default_rng(1).permutation(n)
    V = torch.zeros(n, 128)
    V[:, 0] = torch.from_numpy((perm - n // 2).astype(np.float32))
    label, _, _, sweeps = ops.geomca_components(V.cuda(), n // 2, 1.0)
    assert int(label.max()) == 0
    return sweeps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="4096,16384,100352")
    ap.add_argument("--dense-up-to", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "geomca_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "geomca_bench needs a GPU"
    res = {"metric": "geomca_dense_over_device_end_to_end", "unit": "ratio", "higher_is_better": True,
           "link_sweeps_shuffled_path_4096": path_graph_sweeps()}
    shapes = [int(s) for s in a.shapes.split(",")]
    for n in shapes:
        res[str(n)] = bench_shape(n, a.rounds, n <= a.dense_up_to)
        print(f"# {n}: " + json.dumps(res[str(n)]), file=sys.stderr, flush=True)
    dense = [n for n in shapes if n <= a.dense_up_to]
    res["value"] = res[str(dense[-1])]["dense_over_device_end_to_end"] if dense else None
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
