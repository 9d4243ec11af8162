#!/usr/bin/env python3
"""Time the streaming per-pair top-k over outcomes (csrc/outcome_topk.hip, mdg_outcome_topk_update) against what existed before it
and against a pure read of the same bytes.  Prints one JSON line (recorded as profiles/outcome_topk_bench.json).

    python scripts/outcome_topk_bench.py [--rounds 5] [--parts resident,pipeline] [--out FILE]

Part "resident": x [896, 4096, 4096] resident in HBM, uniform random values standing in for normalised ranks, as fp32 (60 GB) and as
bf16 (30 GB).  Variants per dtype:
  outcome_topk_k1 / _k5 / _k8   one ops.outcome_topk call over all 896 outcomes into a reused state (the fresh fold: what a caller
                                of a resident tensor runs), k = 1, 5, 8
  read_sum                      (b) a pure read of the same bytes: x.sum()
  torch_topk_k5                 (a) what the parent commit could do: torch.topk(x[:, r0:r1], 5, dim=0) over blocks of --block head
                                rows, plus the mean of the values, into the same [5, N, N] / [N, N] results
Part "pipeline": the products end to end on a decoder-only model with random weights (bf16x3 head):
  highest_outcomes_ranks        pipeline.highest_outcomes(of="ranks") at 4096 drugs x 896 outcomes, default max_bytes (chunks of 128)
  rank_all_pairs_only           the same chunks of rank_all_pairs without the fold: what the fold adds is the difference
  ensemble_highest_outcomes     pipeline.ensemble_highest_outcomes with 5 models at 4096 x 158, default max_bytes
  ensemble_ranks_only           the same chunks of rank_all_pairs x 5 + ops.ensemble_ranks without the fold
Part "kernel" (not in the default): three folds of the resident tensor at --k and nothing else, for scripts/outcome_topk_pmc.sh.
All variants of a part run in one process, alternating round by round, timed with HIP events over a window of back-to-back calls
(one pass per round for the variants that take seconds).  ms per pass: median [min, max] over the rounds; TB/s: bytes of x over
the median."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from madrigal_amd import models as M, ops, pipeline  # noqa: E402

N, L, L_ENS, SEEDS = 4096, 896, 158, 5


class DecoderOnly(torch.nn.Module):
    def __init__(self, n_out, seed):
        super().__init__()
        self.decoder = M.BilinearDDIScorer(128, 128, n_out)
        torch.nn.utils.parametrize.register_parametrization(self.decoder, "weight", M.Symmetric())
        with torch.no_grad():
            self.decoder.parametrizations.weight.original.copy_(
                torch.randn(n_out, 128, 128, generator=torch.Generator().manual_seed(seed)) / 128 ** 0.5)


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def run_variants(variants, slow, rounds, slow_rounds, window_s):
    """{name: {"ms", "ms_min_max", "rounds"}} and the calls per window: a warm-up call each, then alternating rounds."""
    reps, times = {}, {v: [] for v in variants}
    for v, fn in variants.items():
        fn()
        torch.cuda.synchronize()
        one = window_ms(fn, 1)
        reps[v] = 1 if v in slow else max(1, math.ceil(window_s * 1e3 / max(one, 1e-3)))
    for rnd in range(rounds):
        for v, fn in variants.items():
            if v in slow and rnd >= slow_rounds:
                continue
            times[v].append(window_ms(fn, reps[v]))
    res = {v: {"ms": round(float(np.median(ts)), 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)], "rounds": len(ts)}
           for v, ts in times.items()}
    return res, reps


def bench_resident(dtype, rounds, slow_rounds, window_s, block):
    x = ops.empty_scores(L, N, N, "cuda", dtype=dtype)
    g = torch.Generator(device="cuda").manual_seed(0)
    for s in range(0, L, 32):                           # filled in slabs: no second 60 GB tensor
        x[s:s + 32] = torch.rand((min(32, L - s), N, N), device="cuda", generator=g).to(dtype)
    nbytes = x.numel() * x.element_size()
    states = {k: ops.outcome_topk(x[:1], k) for k in (1, 5, 8)}
    tk_vals = torch.empty((5, N, N), dtype=dtype, device="cuda")
    tk_idx = torch.empty((5, N, N), dtype=torch.int64, device="cuda")
    tk_mean = torch.empty((N, N), dtype=torch.float32, device="cuda")

    def fold(k):
        vals, idx = states[k]
        from madrigal_amd._lib import call          # a fresh fold into the reused state (ops.outcome_topk allocates a fresh one)
        call("mdg_outcome_topk_update", x.data_ptr(), ops._X_TYPES[dtype], x.stride(0), x.stride(1), None, 0, None, None, vals.data_ptr(),
             idx.data_ptr(), vals.stride(0), vals.stride(1), N, N, L, k, 1, 1, 0, ops._stream(x))

    def torch_topk():
        for r0 in range(0, N, block):
            v, i = torch.topk(x[:, r0:r0 + block], 5, dim=0)
            tk_vals[:, r0:r0 + block], tk_idx[:, r0:r0 + block] = v, i
            tk_mean[r0:r0 + block] = v.float().mean(0)

    variants = {"outcome_topk_k1": lambda: fold(1), "outcome_topk_k5": lambda: fold(5), "outcome_topk_k8": lambda: fold(8),
                "read_sum": lambda: x.sum(dtype=torch.float32), "torch_topk_k5": torch_topk}
    res, reps = run_variants(variants, {"torch_topk_k5"}, rounds, slow_rounds, window_s)
    # the two routes agree (values; torch.topk's order among equal values is unspecified, so the ids are compared where values differ)
    fold(5)
    torch_topk()
    agree = bool(torch.equal(states[5][0], tk_vals.float()))
    out = {"dtype": str(dtype).replace("torch.", ""), "N": N, "L": L, "x_bytes": nbytes, "torch_topk_row_block": block,
           "calls_per_window": reps, "values_equal_torch_topk": agree, "mean_equal_torch_topk": bool(torch.equal(states[5][0].mean(0), tk_mean))}
    out.update(res)
    for v in res:
        out[v]["x_TBps"] = round(nbytes / (res[v]["ms"] * 1e-3) / 1e12, 3)
    for k in (1, 5, 8):
        out[f"k{k}_fraction_of_read_sum"] = round(res["read_sum"]["ms"] / res[f"outcome_topk_k{k}"]["ms"], 3)
    out["torch_topk_k5_over_outcome_topk_k5"] = round(res["torch_topk_k5"]["ms"] / res["outcome_topk_k5"]["ms"], 2)
    del x, states, tk_vals, tk_idx, tk_mean
    torch.cuda.empty_cache()
    return out


def kernel_only(dtype, k, calls):
    """`calls` fresh folds of the resident tensor and nothing else: the workload of a counter pass (scripts/outcome_topk_pmc.sh)."""
    x = ops.empty_scores(L, N, N, "cuda", dtype=dtype)
    g = torch.Generator(device="cuda").manual_seed(0)
    for s in range(0, L, 32):
        x[s:s + 32] = torch.rand((min(32, L - s), N, N), device="cuda", generator=g).to(dtype)
    for _ in range(calls):
        ops.outcome_topk(x, k)
    torch.cuda.synchronize()
    return {"dtype": str(dtype).replace("torch.", ""), "k": k, "calls": calls}


def bench_pipeline(rounds, slow_rounds):
    z = [torch.randn(N, 128, generator=torch.Generator().manual_seed(10 + s)).cuda() for s in range(SEEDS)]
    one = DecoderOnly(L, 0).cuda().eval()
    seeds = [DecoderOnly(L_ENS, 1 + s).cuda().eval() for s in range(SEEDS)]
    plane = N * N * 4
    chunk = (8 << 30) // plane
    chunk_ens = (8 << 30) // ((SEEDS + 2) * plane)
    buf = ops.empty_scores(chunk, N, N, "cuda")

    def ranks_only():
        for s in range(0, L, chunk):
            pipeline.rank_all_pairs(one, z[0], (s, min(L, s + chunk)), out=buf[: min(L, s + chunk) - s])

    def ens_only():
        for s in range(0, L_ENS, chunk_ens):
            e = min(L_ENS, s + chunk_ens)
            ops.ensemble_ranks([pipeline.rank_all_pairs(m, zz, (s, e)) for m, zz in zip(seeds, z)])

    old = M._state["precision"]
    M._state["precision"] = "bf16x3"
    try:
        variants = {"highest_outcomes_ranks": lambda: pipeline.highest_outcomes(one, z[0], 5),
                    "rank_all_pairs_only": ranks_only,
                    "ensemble_highest_outcomes": lambda: pipeline.ensemble_highest_outcomes(seeds, z, 5),
                    "ensemble_ranks_only": ens_only}
        res, reps = run_variants(variants, set(variants), rounds, slow_rounds, 0.0)
    finally:
        M._state["precision"] = old
    out = {"N": N, "L": L, "L_ensemble": L_ENS, "seeds": SEEDS, "precision": "bf16x3", "outcomes_per_chunk": chunk,
           "outcomes_per_ensemble_chunk": chunk_ens}
    out.update(res)
    out["fold_share_of_highest_outcomes"] = round(1 - res["rank_all_pairs_only"]["ms"] / res["highest_outcomes_ranks"]["ms"], 3)
    out["fold_share_of_ensemble_highest_outcomes"] = round(1 - res["ensemble_ranks_only"]["ms"] / res["ensemble_highest_outcomes"]["ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--slow-rounds", type=int, default=2, help="rounds that also run the variants that take seconds per pass")
    ap.add_argument("--window", type=float, default=0.3, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--block", type=int, default=256, help="head rows per torch.topk call of the baseline")
    ap.add_argument("--parts", default="resident,pipeline")
    ap.add_argument("--dtypes", default="float32,bfloat16")
    ap.add_argument("--k", type=int, default=5, help="k of --parts kernel")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "outcome_topk_bench needs a GPU"
    res = {"metric": "outcome_topk_k5_fp32_ms", "unit": "ms", "higher_is_better": False}
    parts = a.parts.split(",")
    if "kernel" in parts:                               # for a counter pass: no timing
        res["kernel"] = [kernel_only(getattr(torch, name), a.k, 3) for name in a.dtypes.split(",")]
    if "resident" in parts:
        for name in a.dtypes.split(","):
            res[f"resident_{name}"] = bench_resident(getattr(torch, name), a.rounds, a.slow_rounds, a.window, a.block)
            print(f"# resident {name}: " + json.dumps(res[f"resident_{name}"]), file=sys.stderr, flush=True)
    if "pipeline" in parts:
        res["pipeline"] = bench_pipeline(max(2, a.slow_rounds), max(2, a.slow_rounds))
        print("# pipeline: " + json.dumps(res["pipeline"]), file=sys.stderr, flush=True)
    if "resident_float32" in res:
        res["value"] = res["resident_float32"]["outcome_topk_k5"]["ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
