#!/usr/bin/env python3
"""Time top-k screening over a checkpoint ensemble (csrc/ensemble_topk.hip, mdg_bilinear_ensemble_topk) against what was possible
before it existed, against its own bare sweep and against the single-model screen.  Prints one JSON line (recorded as
profiles/ensemble_topk_bench.json).

    python scripts/ensemble_topk_bench.py [--rounds 3] [--shapes small,big] [--out FILE]

Shapes: "small" = 4096 x 4096 drugs x 896 outcomes, bf16x3, K in {1, 2, 5} checkpoints, k in {1, 16, 32}, not_self and lower;
"big" = 100 352 x 100 352 x 16, bf16x3, K = 5, k = 16 (at the full 1 024 outcomes no dense route exists: one outcome's [N,N] fp32
plane alone is 40 GB); "full" (not in the default list: about two minutes) = 100 352 x 100 352 x 1 024, K = 5, k = 16, the screen
alone, timed once.  Embeddings are N(0,1) * 0.3 and W ~ N(0,1) / sqrt(128), symmetrised: logits of a few units, no saturated
probabilities, so the lists keep changing through the whole sweep (with saturated inputs they fill with exact ones and the insert
path goes quiet: a cheaper case).  Variants per shape and K:
  ens_topk_{eligible}_k{k}   ops.bilinear_ensemble_topk; k = 1 doubles as (b), the cost of the bare ensemble sweep (one compare per
                             element, an insert about ln(N) times per row)
  dense_topk16               (a) what was possible before: ops.bilinear_ensemble_sigmoid over blocks of head rows sized to a 16 GB
                             buffer, torch.topk(16) over every block (it does not even mask the drug itself)
  single_topk_{eligible}_k{k}   ops.bilinear_topk of ONE model; K times it is (c), a floor that shows what rebuilding T costs
  top_pairs_K1000            pipeline.ensemble_top_pairs(K = 1000) end to end (K = 5)
  ens_topk_not_self_k16_excl1pct   the k = 16 screen with an exclude= mask holding 1 % of all pairs (K = 5)
All variants run in one process, alternating round by round; a round times each variant over a window of at least --window
seconds of back-to-back calls with HIP events (the dense baseline: one pass over all row blocks).  ms per call: median [min, max]
over the rounds."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from madrigal_amd import models as M, ops, pipeline  # noqa: E402

SHAPES = {"small": dict(N=4096, L=896, Ks=(1, 2, 5), ks=(1, 16, 32), modes=("not_self", "lower")),
          "big": dict(N=100_352, L=16, Ks=(5,), ks=(16,), modes=("not_self",))}
PREC = "bf16x3"


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def bench_shape(name, N, L, Ks, ks, modes, rounds, window_s):
    Kmax = max(Ks)
    zs = [(torch.randn(N, 128, generator=torch.Generator().manual_seed(10 + m)) * 0.3).cuda() for m in range(Kmax)]
    raw = [(torch.randn(L, 128, 128, generator=torch.Generator().manual_seed(50 + m)) / 128 ** 0.5).cuda() for m in range(Kmax)]
    ws = [ops.symmetrize(w) for w in raw]
    block = max(1, min(N, (16 << 30) // (L * N * 4)))
    buf = torch.empty(L * block * N, dtype=torch.float32, device="cuda")

    def dense(K):
        def run():
            for r0 in range(0, N, block):
                r1 = min(N, r0 + block)
                p = ops.bilinear_ensemble_sigmoid([z[r0:r1] for z in zs[:K]], zs[:K], ws[:K], precision=PREC,
                                                  out=buf[: L * (r1 - r0) * N].view(L, r1 - r0, N))
                torch.topk(p, 16, dim=2)
        return run

    variants = {}
    for mode in modes:
        for k in ks:
            variants[f"single_topk_{mode}_k{k}"] = (lambda mode=mode, k=k: ops.bilinear_topk(zs[0], zs[0], ws[0], k, eligible=mode, precision=PREC))
    for K in Ks:
        for mode in modes:
            for k in ks:
                variants[f"K{K}_ens_topk_{mode}_k{k}"] = (
                    lambda K=K, mode=mode, k=k: ops.bilinear_ensemble_topk(zs[:K], zs[:K], ws[:K], k, eligible=mode, precision=PREC))
        variants[f"K{K}_dense_topk16"] = dense(K)
    if name == "small":
        g = torch.Generator().manual_seed(3)
        n = N * N // 100
        known = ops.pair_mask(torch.randint(0, N, (n,), generator=g), torch.randint(0, N, (n,), generator=g), N, symmetric=True, device="cuda")
        variants[f"K{Kmax}_ens_topk_not_self_k16_excl1pct"] = (
            lambda: ops.bilinear_ensemble_topk(zs[:Kmax], zs[:Kmax], ws[:Kmax], 16, eligible="not_self", precision=PREC, exclude=known))
        variants[f"K{Kmax}_top_pairs_K1000"] = lambda: pipeline.ensemble_top_pairs(raw[:Kmax], zs[:Kmax], 1000)
    slow = lambda nm: nm.endswith("dense_topk16")      # noqa: E731
    old = M._state["precision"]
    M._state["precision"] = PREC
    try:
        reps, times = {}, {nm: [] for nm in variants}
        for nm, fn in variants.items():               # warm-up, and the number of calls that fills the window
            fn()
            torch.cuda.synchronize()
            one = window_ms(fn, 1)
            reps[nm] = 1 if slow(nm) else max(1, math.ceil(window_s * 1e3 / max(one, 1e-3)))
        for rnd in range(rounds):
            for nm, fn in variants.items():
                times[nm].append(window_ms(fn, reps[nm]))
    finally:
        M._state["precision"] = old
    res = {"N": N, "L": L, "precision": PREC, "z_scale": 0.3, "baseline_row_block": block, "calls_per_window": reps}
    for nm, ts in times.items():
        res[nm] = {"ms": round(float(np.median(ts)), 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)], "rounds": len(ts)}
    ms = lambda nm: res[nm]["ms"]      # noqa: E731
    for K in Ks:
        if 16 in ks:
            res[f"K{K}_dense_topk16_over_ens_topk_k16"] = round(ms(f"K{K}_dense_topk16") / ms(f"K{K}_ens_topk_not_self_k16"), 2)
            res[f"K{K}_ens_topk_k16_over_K_single_topk_k16"] = round(ms(f"K{K}_ens_topk_not_self_k16") / (K * ms("single_topk_not_self_k16")), 3)
    del buf
    torch.cuda.empty_cache()
    return res


def bench_full(N=100_352, L=1024, K=5, k=16, calls=8):
    """The size at which no dense route exists: every outcome of BASELINE configs[4], the screen alone, timed once (no warm-up: the
    kernels run for seconds), as `calls` launches over outcome slices writing into one (vals, idx) pair."""
    zs = [(torch.randn(N, 128, generator=torch.Generator().manual_seed(10 + m)) * 0.3).cuda() for m in range(K)]
    ws = [ops.symmetrize((torch.randn(L, 128, 128, generator=torch.Generator().manual_seed(50 + m)) / 128 ** 0.5).cuda()) for m in range(K)]
    vals = torch.empty((L, N, k), dtype=torch.float32, device="cuda")
    idx = torch.empty((L, N, k), dtype=torch.int32, device="cuda")
    step = L // calls

    def run():
        for s in range(0, L, step):
            ops.bilinear_ensemble_topk(zs, zs, [w[s:s + step] for w in ws], k, eligible="not_self", precision=PREC,
                                       out=(vals[s:s + step], idx[s:s + step]))
    ms = window_ms(run, 1)
    ok = bool(torch.isfinite(vals).all()) and bool(((idx >= 0) & (idx < N)).all())
    return {"N": N, "L": L, "K": K, "k": k, "precision": PREC, "z_scale": 0.3, "launches": calls, "rounds": 1, "warm": False,
            "result_bytes": vals.numel() * 8, "all_entries_valid": ok, f"K{K}_ens_topk_not_self_k{k}": {"ms": round(ms, 1)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.4, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--shapes", default="small,big")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ensemble_topk_bench needs a GPU"
    res = {"metric": "bilinear_ensemble_topk_ms", "unit": "ms", "higher_is_better": False, "device": torch.cuda.get_device_name(0)}
    for name in a.shapes.split(","):
        res[name] = bench_full() if name == "full" else bench_shape(name, rounds=a.rounds, window_s=a.window, **SHAPES[name])
        print(f"# {name}: " + json.dumps(res[name]), file=sys.stderr, flush=True)
    first = a.shapes.split(",")[0]
    res["value"] = res[first]["K5_ens_topk_not_self_k16"]["ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
