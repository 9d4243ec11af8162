#!/usr/bin/env python3
"""Time ops.group_metrics (csrc/eval_metrics.hip, mdg_group_metrics) and metrics.drug_specific_metrics.  Prints one JSON line (recorded
as profiles/drug_metrics_bench.json).

    python scripts/drug_metrics_bench.py [--reps 20] [--out FILE]

Cases (preds = sigmoid(2 y - 1 + N(0, 1))):
  eval3m     data.make_eval_triples(4096, 4096, 896, 1e6): T = 3e6, group = head * 896 + label (~8.8e5 groups of 3-ish triples);
  eval6m     the same generator with 2e6 positives, T = 6e6;
  mid3m      T = 3e6 in groups of 33 to 2048 triples (log-uniform sizes): every group takes the workgroup walk;
  zipf3m     T = 3e6 over 896 groups of Zipf(1.1) sizes (the largest ~5.4e5 triples: one workgroup walks it);
  drug_wall  metrics.drug_specific_metrics on eval3m, wall time including its host reads.
eval3m and mid3m are also timed with every group forced through one walk (MDG_GROUP_WALK = 1 thread, 3 workgroup): the
workloads on each side of the 32-triple cut-off.  Device-event ms: median (min-max) over --reps calls after two warm-ups.
For context only (a CPU figure, not measured here): the reference's sklearn loop took 0.72 s for one drug of 150 labels x 3
triples on one build-machine core, 4.8 ms per (drug, label) group, ~70 min extrapolated to eval3m's ~8.8e5 groups."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from madrigal_amd import data as D, metrics as MT, ops  # noqa: E402
from madrigal_amd._lib import lib  # noqa: E402


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
    return round(float(np.median(out)), 4), [round(float(np.min(out)), 4), round(float(np.max(out)), 4)]


def _pred(y, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.sigmoid(2 * y - 1 + torch.randn(y.numel(), generator=g))


def eval_case(n_pos, seed):
    lab, h, t, pn = D.make_eval_triples(4096, 4096, 896, n_pos, seed)
    return _pred(pn, seed), pn, h * 896 + lab, 4096 * 896, (lab, h, t)


def sized_case(sizes, seed):
    rng = np.random.default_rng(seed)
    group = torch.from_numpy(rng.permutation(np.repeat(np.arange(sizes.size), sizes)).astype(np.int64))
    y = torch.from_numpy((rng.random(group.numel()) < 1 / 3).astype(np.float32))
    return _pred(y, seed), y, group, int(sizes.size), None


def set_walk(v):
    if v is None:
        os.environ.pop("MDG_GROUP_WALK", None)
    else:
        os.environ["MDG_GROUP_WALK"] = str(v)
    lib().mdg_tuning_reload()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "drug_metrics_bench needs a GPU"
    rng = np.random.default_rng(5)
    mid = np.exp(rng.uniform(np.log(33), np.log(2049), 12_000)).astype(np.int64)
    mid = mid[np.cumsum(mid) <= 3_000_000]
    w = 1.0 / np.arange(1, 897) ** 1.1
    zipf = np.bincount(rng.choice(896, 3_000_000, p=w / w.sum()), minlength=896)
    cases = {"eval3m": eval_case(1_000_000, 1), "eval6m": eval_case(2_000_000, 2), "mid3m": sized_case(mid, 3),
             "zipf3m": sized_case(zipf[zipf > 0], 4)}
    res = {"metric": "group_metrics_ms", "targets_ms": {"eval3m": 1.0, "eval6m": 2.0},
           "cpu_reference_context": "reference sklearn get_drug_specific_scores: 4.8 ms per (drug, label) group on one build-machine "
                                    "CPU core, ~70 min extrapolated to eval3m (a CPU extrapolation, not a GPU measurement)"}
    set_walk(None)
    for name, (pred, y, group, n_groups, _) in cases.items():
        args = (pred.cuda(), y.cuda(), group.cuda(), n_groups)
        r = ops.group_metrics(*args, k=50)
        cnt = r["count"]
        res[name] = {"T": int(pred.numel()), "n_groups": n_groups, "groups_present": int(cnt.numel()),
                     "largest_group": int(cnt.max()), "groups_over_32": int((cnt > 32).sum())}
        res[name]["ms"], res[name]["ms_min_max"] = event_ms(lambda: ops.group_metrics(*args, k=50), a.reps)
        if name in ("eval3m", "mid3m"):
            for v, tag in ((1, "thread"), (3, "workgroup")):
                set_walk(v)
                res[name][f"ms_all_{tag}_walk"], _ = event_ms(lambda: ops.group_metrics(*args, k=50), max(5, a.reps // 4))
            set_walk(None)
    pred, y, group, n_groups, (lab, h, t) = cases["eval3m"]
    dev = [x.cuda() for x in (pred, h, t, lab, y)]
    MT.drug_specific_metrics(*dev, 4096, "test_between")
    torch.cuda.synchronize()
    walls = []
    for _ in range(5):
        t0 = time.perf_counter()
        MT.drug_specific_metrics(*dev, 4096, "test_between")
        walls.append((time.perf_counter() - t0) * 1e3)
    res["drug_wall"] = {"T": int(pred.numel()), "drugs": 4096, "wall_ms_median": round(float(np.median(walls)), 2),
                        "wall_ms_min_max": [round(min(walls), 2), round(max(walls), 2)]}
    res["value"] = res["eval3m"]["ms"]
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
