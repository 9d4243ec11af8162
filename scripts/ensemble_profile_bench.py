#!/usr/bin/env python3
"""Time the per-pair outcome profile of a checkpoint ensemble (csrc/ensemble_profile.hip, mdg_bilinear_ensemble_profile) against
what was possible before it existed and against the bare ensemble sweep.  Prints one JSON line (recorded as
profiles/ensemble_profile_bench.json).

    python scripts/ensemble_profile_bench.py [--rounds 3] [--shapes small,big] [--out FILE]
    python scripts/ensemble_profile_bench.py --shapes sizes --out profiles/ensemble_profile_bench_sizes.json

Shapes: "small" = 4096 x 4096 drugs x 896 outcomes, bf16x3, K in {1, 2, 5} checkpoints, every ordered pair ("all") and the lower
triangle ("lower"); "big" = 100 352 x 100 352 x 16, K = 5.  Embeddings are N(0,1) * 0.3 and W ~ N(0,1) / sqrt(128), symmetrised:
logits of a few units, no saturated probabilities.  The cut is P >= 0.9 for every outcome.
Variants per K and eligibility of the small shape:
  profile          ops.bilinear_ensemble_profile
  dense_profile    (a) what was possible before: ops.bilinear_ensemble_sigmoid over blocks of head rows sized to a 16 GB buffer, then
                   (P >= thr).sum(0) and (P - thr).max(0) -- values and argmax in one torch call -- block by block, the upper
                   triangle blanked for "lower" (count and margin checked against the sweep's once; argmax leaves the order of
                   tied outcomes unspecified, so ``best`` is reported as a fraction of agreeing pairs)
  select_count     (b) ops.bilinear_ensemble_select_count at the same cut: the bare ensemble sweep with the outer loops the other
                   way round
  single_x_K       (c) K calls of the single-model ops.bilinear_profile at the cut logit(0.9): a DIFFERENT quantity (K profiles
                   cannot be merged into the ensemble's), here as a yardstick for sweep cost only
The big shape: (d) pipeline.ensemble_most_flagged_pairs(K = 1000 pairs) streamed in 4096-row blocks, as most_flagged_pairs does; the
dense route does not exist there (one outcome's plane is 40 GB).
"sizes": the same number of pair x outcome products at growing N -- 4096 x 896, 8192 x 224, 16 384 x 56, K = 2 -- profile and
select_count on every ordered pair and on the lower triangle: how the cost over the bare sweep and the triangle's saving move with
the number of workgroups in the grid.
All variants run in one process, alternating round by round; a round times each variant over a window of at least --window
seconds of back-to-back calls with HIP events (the dense baseline and the big shape: one call).  ms per call: median [min, max]
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
CUT = 0.9


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def inputs(N, L, K):
    zs = [(torch.randn(N, 128, generator=torch.Generator().manual_seed(10 + m)) * 0.3).cuda() for m in range(K)]
    raw = [(torch.randn(L, 128, 128, generator=torch.Generator().manual_seed(50 + m)) / 128 ** 0.5).cuda() for m in range(K)]
    return zs, raw


def summarise(res, times, reps):
    res["calls_per_window"] = reps
    for nm, ts in times.items():
        res[nm] = {"ms": round(float(np.median(ts)), 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)], "rounds": len(ts)}


def bench_small(N, L, Ks, rounds, window_s):
    Kmax = max(Ks)
    zs, raw = inputs(N, L, Kmax)
    ws = [ops.symmetrize(w) for w in raw]
    thr = torch.full((L,), CUT, device="cuda")
    logit = torch.full((L,), math.log(CUT / (1 - CUT)), device="cuda")
    block = max(1, min(N, (16 << 30) // (L * N * 4)))
    buf = torch.empty(L * block * N, dtype=torch.float32, device="cuda")
    col = torch.arange(N, device="cuda")[None, :]
    t3 = thr[:, None, None]

    def dense(K, eligible, found):
        def run():
            count = torch.empty((N, N), dtype=torch.int32, device="cuda")
            best = torch.empty((N, N), dtype=torch.int64, device="cuda")
            margin = torch.empty((N, N), dtype=torch.float32, device="cuda")
            for r0 in range(0, N, block):
                r1 = min(N, r0 + block)
                p = ops.bilinear_ensemble_sigmoid([z[r0:r1] for z in zs[:K]], zs[:K], ws[:K], precision=PREC,
                                                  out=buf[: L * (r1 - r0) * N].view(L, r1 - r0, N))
                c = (p >= t3).sum(0, dtype=torch.int32)
                m, b = (p - t3).max(0)
                if eligible == "lower":
                    upper = col >= torch.arange(r0, r1, device="cuda")[:, None]      # j >= i: not a pair of the lower triangle
                    c.masked_fill_(upper, 0)
                    b.masked_fill_(upper, -1)
                    m.masked_fill_(upper, float("-inf"))
                count[r0:r1], best[r0:r1], margin[r0:r1] = c, b, m
            found[0] = (count, best, margin)
        return run

    res = {"N": N, "L": L, "precision": PREC, "z_scale": 0.3, "cut": CUT, "baseline_row_block": block,
           "tiles_per_workgroup": ops.bilinear_ensemble_profile_tiles()}
    variants, slow = {}, set()
    for K in Ks:
        for el in ("all", "lower"):
            tag = f"K{K}_{el}"
            c, b, m = ops.bilinear_ensemble_profile(zs[:K], zs[:K], ws[:K], thr, eligible=el, precision=PREC)
            pairs = N * N if el == "all" else N * (N - 1) // 2
            res[f"{tag}_flags_per_pair"] = round(float(c.sum()) / pairs, 4)
            variants[f"{tag}_profile"] = lambda K=K, el=el: ops.bilinear_ensemble_profile(zs[:K], zs[:K], ws[:K], thr, eligible=el, precision=PREC)
            variants[f"{tag}_select_count"] = lambda K=K, el=el: ops.bilinear_ensemble_select_count(zs[:K], zs[:K], ws[:K], thr, eligible=el,
                                                                                                    precision=PREC)

            def singles(K=K, el=el):
                for k in range(K):
                    ops.bilinear_profile(zs[k], zs[k], ws[k], logit, eligible=el, precision=PREC)
            variants[f"{tag}_single_x_K"] = singles
            found = [None]
            variants[f"{tag}_dense_profile"] = dense(K, el, found)
            slow.add(f"{tag}_dense_profile")
            variants[f"{tag}_dense_profile"]()
            dc, db, dm = found[0]
            res[f"{tag}_dense_count_and_margin_agree"] = bool(torch.equal(dc, c) and torch.equal(dm.view(torch.int32), m.view(torch.int32)))
            res[f"{tag}_dense_best_agrees_fraction"] = float((db == b.long()).float().mean())
            found[0] = None
            del c, b, m, dc, db, dm
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
    summarise(res, times, reps)
    ms = lambda nm: res[nm]["ms"]      # noqa: E731
    for K in Ks:
        for el in ("all", "lower"):
            tag = f"K{K}_{el}"
            res[f"{tag}_profile_over_select_count"] = round(ms(f"{tag}_profile") / ms(f"{tag}_select_count"), 3)
            res[f"{tag}_dense_profile_over_profile"] = round(ms(f"{tag}_dense_profile") / ms(f"{tag}_profile"), 2)
            res[f"{tag}_profile_over_single_x_K"] = round(ms(f"{tag}_profile") / ms(f"{tag}_single_x_K"), 3)
    del buf
    torch.cuda.empty_cache()
    return res


def bench_sizes(rounds, window_s, K=2, sizes=((4096, 896), (8192, 224), (16384, 56))):
    res = {"precision": PREC, "z_scale": 0.3, "cut": CUT, "K": K}
    for N, L in sizes:
        zs, raw = inputs(N, L, K)
        ws = [ops.symmetrize(w) for w in raw]
        thr = torch.full((L,), CUT, device="cuda")
        variants = {}
        for el in ("all", "lower"):
            variants[f"N{N}_{el}_profile"] = lambda el=el: ops.bilinear_ensemble_profile(zs, zs, ws, thr, eligible=el, precision=PREC)
            variants[f"N{N}_{el}_select_count"] = lambda el=el: ops.bilinear_ensemble_select_count(zs, zs, ws, thr, eligible=el, precision=PREC)
        reps, times = {}, {nm: [] for nm in variants}
        for nm, fn in variants.items():
            fn()
            torch.cuda.synchronize()
            reps[nm] = max(1, math.ceil(window_s * 1e3 / max(window_ms(fn, 1), 1e-3)))
        for rnd in range(rounds):
            for nm, fn in variants.items():
                times[nm].append(window_ms(fn, reps[nm]))
        part = {}
        summarise(part, times, reps)
        res.setdefault("calls_per_window", {}).update(part.pop("calls_per_window"))
        res.update(part)
        ms = lambda nm: res[nm]["ms"]      # noqa: E731
        res[f"N{N}_L"] = L
        for el in ("all", "lower"):
            res[f"N{N}_{el}_profile_over_select_count"] = round(ms(f"N{N}_{el}_profile") / ms(f"N{N}_{el}_select_count"), 3)
        res[f"N{N}_profile_lower_over_all"] = round(ms(f"N{N}_lower_profile") / ms(f"N{N}_all_profile"), 3)
        res[f"N{N}_select_count_lower_over_all"] = round(ms(f"N{N}_lower_select_count") / ms(f"N{N}_all_select_count"), 3)
        del zs, raw, ws
        torch.cuda.empty_cache()
    return res


def bench_big(N, L, Ks, rounds, window_s):
    K = max(Ks)
    zs, raw = inputs(N, L, K)
    res = {"N": N, "L": L, "precision": PREC, "z_scale": 0.3, "cut": CUT, "K": K, "pairs_kept": 1000, "row_block": 4096}
    old = M._state["precision"]
    M._state["precision"] = PREC
    try:
        fn = lambda: pipeline.ensemble_most_flagged_pairs(raw, zs, CUT, 1000, max_bytes=48 * N * 4096)      # noqa: E731
        top = fn()
        torch.cuda.synchronize()
        res["top_count"], res["kth_count"] = int(top[0][0]), int(top[0][-1])
        times = {"most_flagged_pairs": [window_ms(fn, 1) for _ in range(rounds)]}
    finally:
        M._state["precision"] = old
    summarise(res, times, {"most_flagged_pairs": 1})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.4, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--shapes", default="small,big")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ensemble_profile_bench needs a GPU"
    res = {"metric": "bilinear_ensemble_profile_ms", "unit": "ms", "higher_is_better": False, "device": torch.cuda.get_device_name(0)}
    for name in a.shapes.split(","):
        if name == "sizes":
            res[name] = bench_sizes(rounds=a.rounds, window_s=a.window)
        else:
            res[name] = (bench_small if name == "small" else bench_big)(rounds=a.rounds, window_s=a.window, **SHAPES[name])
        print(f"# {name}: " + json.dumps(res[name]), file=sys.stderr, flush=True)
    first = a.shapes.split(",")[0]
    res["value"] = res[first][{"small": "K5_lower_profile", "big": "most_flagged_pairs", "sizes": "N4096_lower_profile"}[first]]["ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
