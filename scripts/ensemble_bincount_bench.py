#!/usr/bin/env python3
"""Time the counting of a checkpoint ensemble's probabilities between edges (csrc/ensemble_bincount.hip, mdg_bilinear_ensemble_bincount /
_split) against what was possible before it existed and against the bare ensemble sweep.  Prints one JSON line (recorded as
profiles/ensemble_bincount_bench.json).

    python scripts/ensemble_bincount_bench.py [--rounds 3] [--shapes small,big] [--out FILE]

Shapes: "small" = 4096 x 4096 drugs x 896 outcomes, bf16x3, lower triangle, K in {1, 2, 5} checkpoints; "big" = 100 352 x 100 352
x 16, K = 5.  Embeddings are N(0,1) * 0.3 and W ~ N(0,1) / sqrt(128), symmetrised: logits of a few units, no saturated
probabilities.  Two edge sets of 1000 edges per outcome:
  i    the probabilities of pipeline.ensemble_top_pairs(K = 1000), ascending: nearly every pair lies below all edges (fast path)
  ii   1000 evenly spaced edges on [0, 1]: every pair lies between two edges (slow path: a search and an LDS add per element)
Variants per shape and K:
  bincount_{set}         ops.bilinear_ensemble_bincount, lower
  select_count           (b) ops.bilinear_ensemble_select_count at the lowest edge of set i: the parent's count pass, the bare sweep the
                         epilogue rides on
  dense_bincount_{set}   (a) what was possible before: ops.bilinear_ensemble_sigmoid over blocks of head rows sized to a 16 GB buffer,
                         then per outcome torch.bucketize(right=True), the pairs with j >= i sent to a spare bin, and torch.bincount,
                         block by block (checked against the sweep's counts once)
  split_empty_{set}, split_1pct_{set}   (c) split= with an all-zero mask and with a mask holding 1 % of all pairs (small shape, the
                         largest K), against bincount_{set} of the same run
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

SHAPES = {"small": dict(N=4096, L=896, Ks=(1, 2, 5)),
          "big": dict(N=100_352, L=16, Ks=(5,))}
PREC = "bf16x3"
B = 1000


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def bench_shape(name, N, L, Ks, rounds, window_s):
    Kmax = max(Ks)
    zs = [(torch.randn(N, 128, generator=torch.Generator().manual_seed(10 + m)) * 0.3).cuda() for m in range(Kmax)]
    raw = [(torch.randn(L, 128, 128, generator=torch.Generator().manual_seed(50 + m)) / 128 ** 0.5).cuda() for m in range(Kmax)]
    ws = [ops.symmetrize(w) for w in raw]
    block = max(1, min(N, (16 << 30) // (L * N * 4)))
    buf = torch.empty(L * block * N, dtype=torch.float32, device="cuda")
    col = torch.arange(N, device="cuda")[None, :]

    def dense(K, edges, found):
        def run():
            total = torch.zeros((L, B + 2), dtype=torch.int64, device="cuda")
            for r0 in range(0, N, block):
                r1 = min(N, r0 + block)
                p = ops.bilinear_ensemble_sigmoid([z[r0:r1] for z in zs[:K]], zs[:K], ws[:K], precision=PREC,
                                                  out=buf[: L * (r1 - r0) * N].view(L, r1 - r0, N))
                upper = col >= torch.arange(r0, r1, device="cuda")[:, None]          # j >= i: not a pair of the lower triangle
                for l in range(L):
                    b = torch.bucketize(p[l], edges[l], right=True, out_int32=True)
                    b.masked_fill_(upper, B + 1)
                    total[l] += torch.bincount(b.view(-1), minlength=B + 2)
            found[0] = total[:, :B + 1]
        return run

    old = M._state["precision"]
    M._state["precision"] = PREC
    res = {"N": N, "L": L, "precision": PREC, "z_scale": 0.3, "eligible": "lower", "n_edges": B, "baseline_row_block": block}
    try:
        variants, slow = {}, set()
        even = torch.linspace(0.0, 1.0, B, device="cuda")[None, :].expand(L, -1).contiguous()
        for K in Ks:
            top = pipeline.ensemble_top_pairs(raw[:K], zs[:K], B)[0]
            edges = {"i": top.flip(1).contiguous(), "ii": even}
            thr = edges["i"][:, 0].contiguous()
            variants[f"K{K}_select_count"] = lambda K=K, t=thr: ops.bilinear_ensemble_select_count(zs[:K], zs[:K], ws[:K], t, eligible="lower",
                                                                                                 precision=PREC)
            for s, e in edges.items():
                counts = ops.bilinear_ensemble_bincount(zs[:K], zs[:K], ws[:K], e, eligible="lower", precision=PREC)
                res[f"K{K}_fraction_between_edges_{s}"] = float(counts[:, 1:B].sum()) / (L * N * (N - 1) / 2)
                variants[f"K{K}_bincount_{s}"] = lambda K=K, e=e: ops.bilinear_ensemble_bincount(zs[:K], zs[:K], ws[:K], e, eligible="lower",
                                                                                                 precision=PREC)
                found = [None]
                variants[f"K{K}_dense_bincount_{s}"] = dense(K, e, found)
                slow.add(f"K{K}_dense_bincount_{s}")
                variants[f"K{K}_dense_bincount_{s}"]()
                res[f"K{K}_dense_bincount_{s}_agrees"] = bool(torch.equal(found[0], counts))
                found[0] = None
            if K == Kmax and name == "small":
                g = torch.Generator().manual_seed(3)
                n = N * N // 100
                known = ops.pair_mask(torch.randint(0, N, (n,), generator=g), torch.randint(0, N, (n,), generator=g), N, symmetric=True,
                                      device="cuda")
                empty = torch.zeros_like(known)
                for s, e in edges.items():
                    for tag, m in (("empty", empty), ("1pct", known)):
                        variants[f"K{K}_split_{tag}_{s}"] = lambda K=K, e=e, m=m: ops.bilinear_ensemble_bincount(
                            zs[:K], zs[:K], ws[:K], e, eligible="lower", precision=PREC, split=m)
        reps, times = {}, {nm: [] for nm in variants}
        for nm, fn in variants.items():               # warm-up, and the number of calls that fills the window
            if nm in slow:                            # (the dense baseline ran once above, for the agreement check)
                reps[nm] = 1
                continue
            fn()
            torch.cuda.synchronize()
            reps[nm] = max(1, math.ceil(window_s * 1e3 / max(window_ms(fn, 1), 1e-3)))
        for rnd in range(rounds):
            for nm, fn in variants.items():
                times[nm].append(window_ms(fn, reps[nm]))
    finally:
        M._state["precision"] = old
    res["calls_per_window"] = reps
    for nm, ts in times.items():
        res[nm] = {"ms": round(float(np.median(ts)), 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)], "rounds": len(ts)}
    ms = lambda nm: res[nm]["ms"]      # noqa: E731
    for K in Ks:
        for s in ("i", "ii"):
            res[f"K{K}_bincount_{s}_over_select_count"] = round(ms(f"K{K}_bincount_{s}") / ms(f"K{K}_select_count"), 3)
            res[f"K{K}_dense_bincount_{s}_over_bincount_{s}"] = round(ms(f"K{K}_dense_bincount_{s}") / ms(f"K{K}_bincount_{s}"), 2)
            for tag in ("empty", "1pct"):
                if f"K{K}_split_{tag}_{s}" in res:
                    res[f"K{K}_split_{tag}_{s}_over_bincount_{s}"] = round(ms(f"K{K}_split_{tag}_{s}") / ms(f"K{K}_bincount_{s}"), 3)
    del buf
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.4, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--shapes", default="small,big")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ensemble_bincount_bench needs a GPU"
    res = {"metric": "bilinear_ensemble_bincount_ms", "unit": "ms", "higher_is_better": False, "device": torch.cuda.get_device_name(0)}
    for name in a.shapes.split(","):
        res[name] = bench_shape(name, rounds=a.rounds, window_s=a.window, **SHAPES[name])
        print(f"# {name}: " + json.dumps(res[name]), file=sys.stderr, flush=True)
    first = a.shapes.split(",")[0]
    res["value"] = res[first]["K5_bincount_i"]["ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
