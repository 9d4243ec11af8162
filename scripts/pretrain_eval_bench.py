#!/usr/bin/env python3
"""Time the pretraining-evaluation kernels (csrc/retrieval.hip): ops.pair_match_counts at n = 1000 and n = 11 607 (the all-drugs
count), ops.pair_uniformity at m = 11 607, a torch-on-GPU formulation of the same counts (fp32 matmul, comparisons in row chunks)
for comparison, and evaluate.evaluate_pretrain_subsets at the 1000-drug cap on a small model.  Prints one JSON line (recorded as
profiles/pretrain_eval_bench.json).

    python scripts/pretrain_eval_bench.py [--reps 20] [--out FILE]

Device-event ms after two warm-up calls: median, min and max over --reps calls.  Bounds from shapes: the counts do
n^2 D 2 (G) + 2 n^2 D (two triangles) flop, uniformity m^2 D flop, against the 155 TF fp32 matrix rate."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from madrigal_amd import evaluate as E, ops  # noqa: E402

FP32_TFLOPS = 155.0


def event_ms(fn, reps):
    fn()
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(out)), "min_ms": float(np.min(out)), "max_ms": float(np.max(out))}


def torch_counts(X, Y, chunk=2048):
    """The same six counts with torch on the GPU: fp32 matmuls and comparisons in row chunks."""
    n = X.shape[0]
    xh, yh = X / X.norm(dim=1, keepdim=True), Y / Y.norm(dim=1, keepdim=True)
    c = (xh * yh).sum(1)
    nx2, ny2 = (X * X).sum(1), (Y * Y).sum(1)
    d = nx2 + ny2 - 2 * (X * Y).sum(1)
    ar = torch.arange(n, device=X.device)
    out = [torch.zeros(n, dtype=torch.int64, device=X.device) for _ in range(6)]
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        off = ar[lo:hi, None] != ar[None, :]
        C = xh[lo:hi] @ yh.T
        D2 = nx2[lo:hi, None] + ny2[None, :] - 2 * (X[lo:hi] @ Y.T)
        out[0][lo:hi] += ((C > c[lo:hi, None]) & off).sum(1)
        out[1] += ((C > c[None, :]) & off).sum(0)
        out[2][lo:hi] += ((xh[lo:hi] @ xh.T > c[lo:hi, None]) & off).sum(1)
        out[3][lo:hi] += ((yh[lo:hi] @ yh.T > c[lo:hi, None]) & off).sum(1)
        out[4][lo:hi] += ((D2 < d[lo:hi, None]) & off).sum(1)
        out[5] += ((D2 < d[None, :]) & off).sum(0)
    return out


def subsets_case(reps):
    from madrigal_amd import data as D, models as M
    from oracle.params import det_state_dict
    from test_pretrain_gpu import _build
    from test_pretrain_eval_gpu import Collator
    n, seed = 1400, 3
    masks = D.make_masks(n, seed, p_kg=0.9, p_cv=0.3, p_tx=0.1)
    batch, bkg = D.make_batch(n, seed, kg_nodes=3000, kg_edges=30000, masks=masks)
    model = _build(M, bkg["data"], False, True, mlp_dim=512, T=0.1)
    sd = model.state_dict()
    model.load_state_dict(det_state_dict(seed, {k: tuple(v.shape) for k, v in sd.items()}))
    model = model.cuda().eval()
    col = Collator(batch, {"data": bkg["data"], "drug_index_map": bkg["drug_index_map"]})
    drugs, mk = np.arange(n), masks.numpy().astype(np.int64)
    np.random.seed(0)
    run = lambda: E.evaluate_pretrain_subsets(model, drugs, mk, None, col, [0], [1], "cuda", max_drugs=1000)
    t = event_ms(run, reps)
    ids = np.random.choice(np.flatnonzero((1 - mk[:, [0, 1]]).sum(1) == 2), 1000, replace=False)
    t["collator_ms"] = event_ms(lambda: col([ids]), reps)["median_ms"]      # the test collator's per-drug Python gather, inside the above
    xs = [torch.randn(1000, 128, device="cuda") for _ in range(4)]
    t["metrics_only_ms"] = event_ms(lambda: [E.RT.topk_from_counts(E.RT.pair_counts(a, b), [("one", 20), ("both", 20)])
                                              for a, b in ((xs[0], xs[1]), (xs[2], xs[3]))], reps)["median_ms"]
    t["n_valid"] = int(((1 - mk[:, [0, 1]]).sum(1) == 2).sum())
    t["n_used"] = min(1000, t["n_valid"])
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="only the HIP calls (for a kernel-trace run)")
    a = ap.parse_args()
    torch.manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps}
    for n in (1000, 11607):
        X = torch.randn(n, 128, device="cuda")
        Y = X + 2.0 * torch.randn(n, 128, device="cuda")
        t = event_ms(lambda: ops.pair_match_counts(X, Y), a.reps)
        flop = 4.0 * n * n * 128
        t["bound_ms"] = flop / (FP32_TFLOPS * 1e12) * 1e3
        t["tflops_at_median"] = flop / (t["median_ms"] * 1e-3) / 1e12
        res[f"pair_match_counts_n{n}"] = t
        if not a.kernels_only:
            res[f"torch_counts_n{n}"] = event_ms(lambda: torch_counts(X, Y), max(3, a.reps // 4))
            got = ops.pair_match_counts(X, Y)
            ref = torch_counts(X, Y)
            res[f"torch_counts_n{n}"]["max_count_diff"] = int(max((got[k].long() - r).abs().max() for k, r in
                                                                  zip(("cos_row", "cos_col", "same_x", "same_y", "dist_row", "dist_col"), ref)))
    m = 11607
    X = torch.randn(m, 128, device="cuda")
    t = event_ms(lambda: ops.pair_uniformity(X), a.reps)
    t["bound_ms"] = 1.0 * m * m * 128 / (FP32_TFLOPS * 1e12) * 1e3
    res[f"pair_uniformity_m{m}"] = t
    if not a.kernels_only:
        xh = X / X.norm(dim=1, keepdim=True)
        res[f"torch_uniformity_m{m}"] = event_ms(lambda: torch.pdist(xh).pow(2).mul(-2).exp().mean().log(), max(3, a.reps // 4))
        res["evaluate_pretrain_subsets_cap1000"] = subsets_case(max(3, a.reps // 4))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
