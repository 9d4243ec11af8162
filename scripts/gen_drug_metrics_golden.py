#!/usr/bin/env python3
"""Record tests/golden/drug_metrics.npz from the REFERENCE's own get_drug_specific_scores (madrigal/evaluate/predict.py:274-355).

TEST INFRASTRUCTURE ONLY: needs a checkout of the reference and sklearn; no GPU.
    python scripts/gen_drug_metrics_golden.py --ref <reference checkout> [--out tests/golden/drug_metrics.npz]

predict.py imports the model stack, so it is not imported: the file is parsed with ``ast`` and only get_drug_specific_scores is
executed (as scripts/gen_pretrain_eval_golden.py does), with the reference's get_metrics (madrigal/evaluate/metrics.py, loaded
through the sklearn keyword shim of scripts/gen_eval_metrics_golden.py) and a stub make_predictions that returns the stored
probabilities.  Cases (collator val/test layout: positives, then two aligned negative blocks):
  between / between_train   300 head drugs, 400 tail drugs, 200 labels, 1 500 positives, in both modes;
  ties                      scores quantised to 1/16 (groups stay under 50 triples, so no k-th place exists to tie at);
  mixed                     drug 0 mixes groups of 3 to 90 triples, drug 1 has only groups of 51 or more (its @50 metrics are
                            defined); the k-th place of every group of 50 or more lies outside a run of tied scores;
  err_*                     the reference's failures: a head drug without positives, a (drug, label) problem of one class (a
                            negative relabelled, preds all below 0.5), and too few negatives.
"""
from __future__ import annotations

import argparse
import ast
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_eval_metrics_golden import load_reference_metrics  # noqa: E402

MODES = {"between": "test_between", "between_train": "test_between_train", "ties": "test_between", "mixed": "test_between"}


def load_reference(ref_root: str, preds_box: dict):
    metrics = load_reference_metrics(ref_root)
    rel = os.path.join("madrigal", "evaluate", "predict.py")
    tree = ast.parse(open(os.path.join(ref_root, rel)).read())
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "get_drug_specific_scores"]
    assert len(defs) == 1
    ns = {"np": np, "torch": torch, "get_metrics": metrics.get_metrics,
          "make_predictions": lambda *a, **kw: torch.from_numpy(preds_box["preds"].copy())}
    exec(compile(ast.Module(body=defs, type_ignores=[]), rel, "exec"), ns)
    return ns["get_drug_specific_scores"]


def layout(lab, h, t, n1, n2):
    n = lab.size
    return (np.concatenate([lab, lab, lab]), np.concatenate([h, h, h]), np.concatenate([t, n1, n2]),
            np.concatenate([np.ones(n), np.zeros(2 * n)]).astype(np.float32))


def random_case(rng, n_head, n_tail, L, n_pos, quant=None):
    lab = rng.integers(0, L, n_pos)
    h = rng.integers(0, n_head, n_pos)
    h[rng.permutation(n_pos)[:n_head]] = np.arange(n_head)
    t, n1, n2 = (rng.integers(0, n_tail, n_pos) for _ in range(3))
    labels, heads, tails, pn = layout(lab, h, t, n1, n2)
    p = np.clip(0.3 * pn + 0.7 * rng.random(pn.size), 0, 1)
    if quant:
        p = np.round(p * quant) / quant
    return labels, heads, tails, pn, p.astype(np.float32)


def untie_at_k(preds, groups, k=50):
    """Spread the run of equal scores at the k-th place of each group of more than k triples (steps of 2^-20)."""
    for g in np.unique(groups):
        idx = np.flatnonzero(groups == g)
        if idx.size <= k:
            continue
        s = np.sort(preds[idx])[::-1]
        if s[k - 1] != s[k]:
            continue
        grp = idx[preds[idx] == s[k - 1]]
        preds[grp] = (s[k - 1] - np.arange(grp.size) * 2.0 ** -20).astype(np.float32)
    return preds


def mixed_case(rng):
    n_head, n_tail, L = 4, 60, 12
    sizes = {0: [1, 2, 5, 17, 30, 1, 3, 11], 1: [17, 20, 25], 2: [1, 1], 3: [2]}     # positives per label of each head drug
    lab, h = [], []
    for d, per_label in sizes.items():
        for l, c in enumerate(per_label):
            lab += [l] * c
            h += [d] * c
    lab, h = np.array(lab), np.array(h)
    perm = rng.permutation(lab.size)
    lab, h = lab[perm], h[perm]
    t, n1, n2 = (rng.integers(0, n_tail, lab.size) for _ in range(3))
    labels, heads, tails, pn = layout(lab, h, t, n1, n2)
    p = np.clip(0.3 * pn + 0.7 * rng.random(pn.size), 0, 1)
    p = (np.round(p * 64) / 64).astype(np.float32)
    p = untie_at_k(p, heads * L + labels)
    return n_head, n_tail, labels, heads, tails, pn, p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "drug_metrics.npz"))
    a = ap.parse_args()
    import warnings
    warnings.simplefilter("ignore")
    box = {}
    ref = load_reference(a.ref, box)
    rng = np.random.default_rng(2024)
    cases = {}
    base = random_case(rng, 300, 400, 200, 1500)
    cases["between"] = (300, 400) + base
    cases["between_train"] = (300, 400) + base
    cases["ties"] = (120, 150) + random_case(rng, 120, 150, 40, 900, quant=16)
    cases["mixed"] = mixed_case(rng)
    # error cases
    e_lab, e_h, e_t, e_pn, e_p = random_case(rng, 20, 30, 6, 60)
    h_nopos = e_h.copy()
    h_nopos[e_h == 7] = 8                                               # head drug 7 loses its positives (and their negatives)
    cases["err_nopos"] = (20, 30, e_lab, h_nopos, e_t, e_pn, e_p)
    lab1 = e_lab.copy()
    p1 = e_p.copy()
    i = 60 + int(np.flatnonzero(e_h[:60] == 3)[0])                      # a first negative of head drug 3 ...
    lab1[i] = 6                                                         # ... under a label no positive of drug 3 has
    p1[i] = 0.25
    cases["err_oneclass"] = (20, 30, lab1, e_h, e_t, e_pn, p1)
    cases["err_short"] = (20, 30, e_lab[:-5], e_h[:-5], e_t[:-5], e_pn[:-5], e_p[:-5])

    out = {}
    for name, (n_head, n_tail, labels, heads, tails, pn, preds) in cases.items():
        mode = MODES.get(name, "test_between")
        batch = {"edge_indices": {"head": torch.from_numpy(heads.astype(np.int64)), "tail": torch.from_numpy(tails.astype(np.int64)),
                                  "label": torch.from_numpy(labels.astype(np.int64)), "pos_neg": torch.from_numpy(pn)},
                 "head": {"drugs": torch.arange(n_head) + 10_000}, "tail": {"drugs": torch.arange(n_tail) + 20_000}}
        box["preds"] = preds
        out[f"{name}/labels"], out[f"{name}/heads"], out[f"{name}/tails"] = (x.astype(np.int16) for x in (labels, heads, tails))
        out[f"{name}/pos_neg"], out[f"{name}/preds"] = pn.astype(np.int8), preds
        out[f"{name}/n_head_tail"] = np.array([n_head, n_tail])
        out[f"{name}/mode"] = np.array(mode)
        try:
            res, drugs = ref(None, batch, "full_full", None, "cpu", mode=mode)
        except Exception as exc:                                        # noqa: BLE001 -- what the reference raises is the record
            out[f"{name}/exception"] = np.array(type(exc).__name__)
            print(name, mode, "raises", type(exc).__name__, exc)
            continue
        out[f"{name}/names"] = np.array(list(res.keys()))
        out[f"{name}/values"] = np.array([[np.float64(v) for v in vs] for vs in res.values()])
        out[f"{name}/drugs"] = np.asarray(drugs, dtype=np.int64)
        v = out[f"{name}/values"]
        print(name, mode, "drugs", v.shape[1], "NaN fraction per metric", np.round(np.isnan(v).mean(axis=1), 3))
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
