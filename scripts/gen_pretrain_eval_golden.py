#!/usr/bin/env python3
"""Record tests/golden/pretrain_eval.npz from the REFERENCE's own pretraining-evaluation metrics.

TEST INFRASTRUCTURE ONLY: needs a checkout of the reference; no GPU.
    python scripts/gen_pretrain_eval_golden.py --ref <reference checkout> [--out tests/golden/pretrain_eval.npz]

The reference modules import torch_geometric, torchdrug and GeomCA, so they are not imported: their files are parsed with ``ast``
and only these function definitions are executed (as oracle/gen_golden.py does): uniform_loss, alignment_loss, foscttm and
stacked_inst_dist_topk_accuracy (madrigal/evaluate/eval_utils.py), get_inst_dist_topk_accuracy (madrigal/evaluate/evaluate.py)
and from_indices_to_tensor (madrigal/utils.py).

Cases: n in {20, 257, 1000}, D = 128, Y = X + noise.  Inputs are stored as float16 (upcast to fp32 exactly in the tests).  No
comparison lies within 1e-4 of its threshold (tests/pretrain_eval_ref.py's near-tie count): the rows of Y involved in a near-tie
are redrawn, so every decision is the same under any fp32 rounding.
"""
from __future__ import annotations

import argparse
import ast
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import pretrain_eval_ref as R  # noqa: E402

FUNCS = {os.path.join("madrigal", "evaluate", "eval_utils.py"): ["uniform_loss", "alignment_loss", "foscttm",
                                                                 "stacked_inst_dist_topk_accuracy"],
         os.path.join("madrigal", "evaluate", "evaluate.py"): ["get_inst_dist_topk_accuracy"],
         os.path.join("madrigal", "utils.py"): ["from_indices_to_tensor"]}
CASES = ((20, 7.0, 1), (257, 4.0, 2), (1000, 3.0, 3))           # (n, noise scale, seed)


def load_reference(ref_root: str) -> dict:
    import typing
    ns = {"torch": torch, "np": np, "Iterable": typing.Iterable, "Union": typing.Union}
    for rel, names in FUNCS.items():
        tree = ast.parse(open(os.path.join(ref_root, rel)).read())
        defs = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in names]
        assert sorted(d.name for d in defs) == sorted(names), (rel, [d.name for d in defs])
        exec(compile(ast.Module(body=defs, type_ignores=[]), rel, "exec"), ns)
    return ns


def _ambiguous_rows(X, Y, rel=1e-4) -> np.ndarray:
    c = R.counts(X, Y, rel=rel)
    bad = np.zeros(X.shape[0], dtype=bool)
    for name in R.COUNT_NAMES:
        bad |= c["amb_" + name] > 0
    return np.flatnonzero(bad)


def make_case(n: int, sigma: float, seed: int):
    rng = np.random.default_rng([seed, 2024])
    X = (rng.standard_normal((n, 128)) / np.sqrt(128)).astype(np.float16)
    noise = lambda m: rng.standard_normal((m, 128)) * sigma / np.sqrt(128)
    Y = (X.astype(np.float64) + noise(n)).astype(np.float16)
    for _ in range(50):
        bad = _ambiguous_rows(X.astype(np.float32), Y.astype(np.float32))
        if bad.size == 0:
            return X, Y
        Y[bad] = (X[bad].astype(np.float64) + noise(bad.size)).astype(np.float16)
    raise RuntimeError(f"n={n}: near-ties remain after 50 redraws")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "pretrain_eval.npz"))
    a = ap.parse_args()
    ref = load_reference(a.ref)
    out = {}
    for n, sigma, seed in CASES:
        X16, Y16 = make_case(n, sigma, seed)
        X, Y = torch.from_numpy(X16.astype(np.float32)), torch.from_numpy(Y16.astype(np.float32))
        tag = f"n{n}"
        out[tag + "_x"], out[tag + "_y"] = X16, Y16
        acc, both = [], None
        for k in (1, 5, 20):
            topk_acc, top20, top5, top1, _, _ = ref["get_inst_dist_topk_accuracy"](X, Y, k, "cosine")
            acc.append(topk_acc)
            both = (top20, top5, top1)
        out[tag + "_acc_k1_5_20"] = np.array(acc, dtype=np.float64)
        out[tag + "_stacked_top20_5_1"] = np.array(both, dtype=np.float64)
        mu_xy, std_xy = ref["foscttm"](X, Y)
        mu_yx, std_yx = ref["foscttm"](Y, X)
        out[tag + "_foscttm_xy"] = np.array([float(mu_xy), float(std_xy)])
        out[tag + "_foscttm_yx"] = np.array([float(mu_yx), float(std_yx)])
        out[tag + "_uniform_x_y"] = np.array([float(ref["uniform_loss"](X)), float(ref["uniform_loss"](Y))])
        out[tag + "_alignment"] = np.array([float(ref["alignment_loss"](X, Y))])
        print(tag, "acc k=1,5,20", acc, "stacked", both, "foscttm", out[tag + "_foscttm_xy"], "uniform", out[tag + "_uniform_x_y"])
    out["cases"] = np.array([c[0] for c in CASES], dtype=np.int64)
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
