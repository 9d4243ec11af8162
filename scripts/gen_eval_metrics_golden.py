#!/usr/bin/env python3
"""Record tests/golden/eval_metrics.npz from the REFERENCE's own madrigal/evaluate/metrics.py (get_metrics / get_metrics_binary).

TEST INFRASTRUCTURE ONLY: needs a checkout of the reference and sklearn; no GPU.
    python scripts/gen_eval_metrics_golden.py --ref <reference checkout> [--out tests/golden/eval_metrics.npz]

The reference module is loaded from its file alone (its package __init__ pulls in the model stack).  sklearn >= 1.5 renamed
precision_recall_curve's ``probas_pred`` to ``y_score`` (and 1.7 removed the old name), which the reference's fmax_score still
passes: a one-line shim maps the keyword back.

Every case keeps the k-th place of each label outside a run of tied scores, so the reference's unstable np.argsort cannot change
the recorded top-k metrics; ties elsewhere (scores quantised to 1/64, saturated 1.0) are kept on purpose.
"""
from __future__ import annotations

import argparse
import importlib.util
import os

import numpy as np


def load_reference_metrics(ref_root: str):
    import sklearn.metrics as skm
    spec = importlib.util.spec_from_file_location("ref_metrics", os.path.join(ref_root, "madrigal", "evaluate", "metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.precision_recall_curve = lambda y_true, probas_pred, pos_label=None: skm.precision_recall_curve(y_true, probas_pred, pos_label=pos_label)
    return mod


def _untie_at_k(preds, labels, k, ks_for_label):
    """Spread the run of equal scores that straddles each label's k-th place over distinct values (steps of 2^-20, inside one
    1/64 quantum), so that the top k is the same set under any tie order."""
    for l in np.unique(labels):
        idx = np.flatnonzero(labels == l)
        kk = ks_for_label(len(idx))
        if kk >= len(idx):
            continue
        s = np.sort(preds[idx])[::-1]
        if s[kk - 1] != s[kk]:
            continue
        grp = idx[preds[idx] == s[kk - 1]]
        preds[grp] = (s[kk - 1] - np.arange(len(grp), dtype=np.float64) * 2.0 ** -20).astype(np.float32)
    return preds


def make_case(seed, T, L, zipf, absent, quant, k, one_class_labels=True, one_problem=False):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, L + 1) ** zipf
    w[list(absent)] = 0.0
    w /= w.sum()
    labels = rng.choice(L, size=T, p=w)
    present = np.unique(labels)
    small = [l for l in present if (labels == l).sum() < 12]
    labels[np.isin(labels, small)] = present[0]                   # every problem has >= 12 triples: both rounded classes appear
    rate = rng.uniform(0.05, 0.6, L)
    ys = (rng.random(T) < rate[labels]).astype(np.float32)
    pr = np.clip(0.35 * ys + 0.65 * rng.random(T), 0, 1)
    if quant:
        pr = np.round(pr * 64) / 64
        pr[rng.random(T) < 0.05] = 1.0                             # saturated sigmoid
    preds = pr.astype(np.float32)
    if one_class_labels:
        present = np.unique(labels)
        ys[labels == present[1]] = 0.0                             # all-negative label
        ys[labels == present[2]] = 1.0                             # all-positive label
    ks = (lambda n: int(k * n)) if isinstance(k, float) else (lambda n: k)
    groups = np.zeros_like(labels) if one_problem else labels       # micro / binary: the top k of all triples
    preds = _untie_at_k(preds, groups, k, ks)
    for l in np.unique(labels):                                    # both rounded classes inside every label (no 1 x 1 confusion)
        idx = np.flatnonzero(labels == l)
        preds[idx[0]], preds[idx[1]] = 0.125, 0.875
    preds = _untie_at_k(preds, groups, k, ks)
    return preds, ys, labels.astype(np.int64)


CASES = [
    # name, seed, T, L, zipf, absent labels, quantised, k, [(task, average), ...]
    ("skewed", 1, 12000, 48, 1.1, (5, 17, 40), True, 50, [("multilabel", None), ("multilabel", "macro"), ("multilabel", "weighted")]),
    ("fraction", 2, 6000, 10, 0.6, (), True, 0.1, [("multilabel", None), ("multilabel", "macro")]),
    ("k_over_n", 3, 4000, 24, 1.3, (3,), False, 200, [("multilabel", None), ("multilabel", "macro")]),
    ("micro", 4, 5000, 16, 0.8, (), True, 100, [("multilabel", "micro")]),
    ("binary", 5, 3000, 1, 0.0, (), True, 0.05, [("binary", "macro")]),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of a reference checkout (holds madrigal/evaluate/metrics.py)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "eval_metrics.npz"))
    a = ap.parse_args()
    import warnings
    warnings.simplefilter("ignore")
    ref = load_reference_metrics(a.ref)
    out = {}
    for name, seed, T, L, zipf, absent, quant, k, runs in CASES:
        preds, ys, labels = make_case(seed, T, L, zipf, absent, quant, k, one_class_labels=L >= 3,
                                       one_problem=any(t == "binary" or v == "micro" for t, v in runs))
        out[f"{name}/preds"], out[f"{name}/ys"], out[f"{name}/labels"] = preds, ys, labels.astype(np.int16)
        out[f"{name}/k"] = np.array(k)
        for task, avg in runs:
            tag = f"{name}/{task}/{avg}"
            d, pos = ref.get_metrics(preds, ys, labels, k=k, task=task, average=avg, verbose=False)
            out[f"{tag}/names"] = np.array(list(d.keys()))
            out[f"{tag}/values"] = np.array([np.asarray(v, dtype=np.float64) for v in d.values()])
            out[f"{tag}/pos"] = np.asarray(pos, dtype=np.float64)
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out} ({os.path.getsize(a.out) / 1e3:.0f} kB, {len(CASES)} cases)")


if __name__ == "__main__":
    main()
