#!/usr/bin/env python3
"""Record tests/golden/knn.npz from the REFERENCE's own kNN classifier.

TEST INFRASTRUCTURE ONLY: needs a checkout of the reference and scipy; no GPU.
    python scripts/gen_knn_golden.py --ref <reference checkout> [--out tests/golden/knn.npz]

The reference module imports torch_geometric and torchdrug, so it is not imported: its file is parsed with ``ast`` and only
``knn_classifier`` (madrigal/evaluate/eval_utils.py) is executed, with ``scipy.spatial.distance_matrix`` in its namespace (as
scripts/gen_pretrain_eval_golden.py does for the retrieval metrics).

Cases: (train, test) sizes (300, 77) and (1000, 257), D = 128; k in {1, 5, 20}, metric in {cosine, euclidean}, T in {0.07, 1},
num_classes in {2, 4}.  Inputs are clustered (8 centres; the class of a drug is its centre modulo num_classes, 15 % of the labels
redrawn) and lie on a grid of 1/32, stored as float16 (upcast to fp32 exactly in the tests; the coarse grid is what keeps the
compressed file small).  They are scaled so that every distance stays below 88 * 0.07: the reference weights Euclidean neighbours
by exp(+distance / T), which fp32 holds only up to e^88.

Condition on the inputs (checked here with tests/knn_ref.py, test rows redrawn at most 50 times): no test query is ambiguous at
tol = 1e-4 for any (metric, k), and no vote margin is under 1e-3 of its weight sum, so every neighbour set and every prediction
is the same under any fp32 rounding.  The recorded accuracies are the reference's; knn_ref must reproduce them (asserted).
"""
from __future__ import annotations

import argparse
import ast
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import knn_ref as R  # noqa: E402

SIZES = ((300, 77, 11), (1000, 257, 12))                 # (train, test, seed)
KS, METRICS, TS, CLASSES = (1, 5, 20), ("cosine", "euclidean"), (0.07, 1.0), (2, 4)
CENTRES, GRID = 8, 32.0
AMBIGUOUS_TOL, MIN_MARGIN = 1e-4, 1e-3


def load_reference(ref_root: str) -> dict:
    from scipy.spatial import distance_matrix
    ns = {"torch": torch, "np": np, "distance_matrix": distance_matrix}
    rel = os.path.join("madrigal", "evaluate", "eval_utils.py")
    tree = ast.parse(open(os.path.join(ref_root, rel)).read())
    defs = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == "knn_classifier"]
    assert len(defs) == 1, rel
    exec(compile(ast.Module(body=defs, type_ignores=[]), rel, "exec"), ns)
    return ns


def case_key(ntr, k, metric, T, nc) -> str:
    return f"n{ntr}_k{k}_{metric}_T{T:g}_c{nc}"


def _draw(rng, centres, n):
    c = rng.integers(0, CENTRES, n)
    x = centres[c] + 0.15 * rng.standard_normal((n, 128))
    return (np.round(x * GRID) / GRID).astype(np.float16), c


def _labels(rng, c, nc):
    lab = c % nc
    flip = rng.random(c.size) < 0.15
    lab[flip] = rng.integers(0, nc, int(flip.sum()))
    return lab.astype(np.uint8)


def bad_rows(train, test, labels) -> np.ndarray:
    tr, te = train.astype(np.float32), test.astype(np.float32)
    bad = np.zeros(te.shape[0], dtype=bool)
    for metric in METRICS:
        for k in KS:
            bad[R.ambiguous(te, tr, k, metric, AMBIGUOUS_TOL)] = True
            vals, idx = R.topk(te, tr, k, metric)
            for T in TS:
                for nc in CLASSES:
                    margin = R.vote(vals, idx, labels[nc], T, nc)[2]
                    bad |= margin < MIN_MARGIN
    return np.flatnonzero(bad)


def make_case(ntr: int, nte: int, seed: int):
    rng = np.random.default_rng([seed, 2025])
    centres = 0.2 * rng.standard_normal((CENTRES, 128))
    train, ctr = _draw(rng, centres, ntr)
    test, cte = _draw(rng, centres, nte)
    labels = {nc: _labels(rng, ctr.copy(), nc) for nc in CLASSES}
    for _ in range(50):
        bad = bad_rows(train, test, labels)
        if bad.size == 0:
            return train, test, ctr, cte, labels
        test[bad], cte[bad] = _draw(rng, centres, bad.size)
    raise RuntimeError(f"({ntr}, {nte}): ambiguous queries remain after 50 redraws")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "knn.npz"))
    a = ap.parse_args()
    ref = load_reference(a.ref)["knn_classifier"]
    out = {"sizes": np.array([s[:2] for s in SIZES], dtype=np.int64)}
    for ntr, nte, seed in SIZES:
        train, test, ctr, cte, labels = make_case(ntr, nte, seed)
        rng = np.random.default_rng([seed, 7])
        tag = f"n{ntr}"
        out[tag + "_train"], out[tag + "_test"] = train, test
        ttr, tte = torch.from_numpy(train.astype(np.float32)), torch.from_numpy(test.astype(np.float32))
        assert float(np.sqrt(R.keys(tte, ttr, "euclidean").max())) < 88 * min(TS)
        for nc in CLASSES:
            test_lab = _labels(rng, cte.copy(), nc)
            out[f"{tag}_train_labels_c{nc}"], out[f"{tag}_test_labels_c{nc}"] = labels[nc], test_lab
            for metric in METRICS:
                for k in KS:
                    vals, idx = R.topk(tte.numpy(), ttr.numpy(), k, metric)
                    for T in TS:
                        acc = ref(ttr, torch.from_numpy(labels[nc].astype(np.int64)), tte, torch.from_numpy(test_lab.astype(np.int64)),
                                  metric=metric, k=k, T=T, num_classes=nc)
                        mine = float((R.vote(vals, idx, labels[nc], T, nc)[0] == test_lab).sum()) / nte
                        assert acc == mine, (case_key(ntr, k, metric, T, nc), acc, mine)
                        out[case_key(ntr, k, metric, T, nc)] = np.array(acc, dtype=np.float64)
        print(tag, {k: float(v) for k, v in out.items() if k.startswith(tag + "_k") and k.endswith("c4")})
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
