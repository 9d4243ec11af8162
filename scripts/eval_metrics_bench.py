#!/usr/bin/env python3
"""Time ops.label_metrics (csrc/eval_metrics.hip) at the finetune size -- T = 6e6 labelled triples over L = 896 outcomes, uniform and
Zipf label sizes -- beside the existing torch-based metrics.macro_auprc on the same inputs, and evaluate.evaluate_ddi end to end on
a small model.  Prints one JSON line (recorded as profiles/eval_metrics_bench.json).

    python scripts/eval_metrics_bench.py [--reps 20] [--out FILE]

Device-event ms: median over --reps calls after two warm-up calls.  Algorithmic bytes: T x 16 B in (pred, target, label) plus the
outputs ([13, L] f64 and three [L] int64); GB/s against the 8 TB/s HBM peak.  For context only (not measured here): the reference's
sklearn get_metrics took 4.0 s for 6e5 triples over 896 outcomes on one core of a build machine's CPU (~40 s extrapolated to 6e6)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from madrigal_amd import metrics as MT, ops  # noqa: E402

PEAK_GBS = 8000.0


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
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def inputs(T, L, dist, seed):
    g = torch.Generator().manual_seed(seed)
    if dist == "uniform":
        lab = torch.randint(0, L, (T,), generator=g)
    else:
        w = 1.0 / torch.arange(1, L + 1, dtype=torch.float64) ** 1.1
        lab = torch.multinomial(w, T, replacement=True, generator=g)
    y = (torch.rand(T, generator=g) < 1 / 3).float()
    pred = torch.sigmoid(2 * y - 1 + torch.randn(T, generator=g))
    return pred.cuda(), y.cuda(), lab.cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--T", type=int, default=6_000_000)
    ap.add_argument("--L", type=int, default=896)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-torch-baseline", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "eval_metrics_bench needs a GPU"
    T, L = a.T, a.L
    res = {"metric": "label_metrics_ms", "T": T, "L": L, "target_ms_uniform": 2.0, "hbm_peak_GBs": PEAK_GBS,
           "cpu_reference_context": "reference sklearn get_metrics: 4.0 s for 6e5 triples / 896 outcomes, one build-machine CPU core "
                                    "(not a GPU measurement)"}
    nbytes = T * 16 + L * (13 * 8 + 3 * 8)
    for dist in ("uniform", "zipf"):
        pred, y, lab = inputs(T, L, dist, 1)
        med, lo, hi = event_ms(lambda: ops.label_metrics(pred, y, lab, L, k=50), a.reps)
        res[f"{dist}_ms"] = round(med, 4)
        res[f"{dist}_ms_min_max"] = [round(lo, 4), round(hi, 4)]
        res[f"{dist}_GBs"] = round(nbytes / med / 1e6, 1)
        res[f"{dist}_peak_fraction"] = round(nbytes / med / 1e6 / PEAK_GBS, 4)
        res[f"{dist}_largest_label"] = int(torch.bincount(lab, minlength=L).max())
        t0 = time.perf_counter()
        d, _ = MT.get_metrics(pred, y, lab, k=50, verbose=False)
        res[f"{dist}_get_metrics_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        if not a.no_torch_baseline:
            med_t, _, _ = event_ms(lambda: MT.macro_auprc(pred, y, lab, L), max(3, a.reps // 5))
            res[f"{dist}_torch_macro_auprc_ms"] = round(med_t, 2)
    res["algorithmic_bytes"] = nbytes
    res["value"] = res["uniform_ms"]
    res["unit"] = "ms"
    res["higher_is_better"] = False
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
