#!/usr/bin/env python3
"""Time the split counting sweep (the SPLIT instantiations of csrc/bincount.hip, mdg_bilinear_bincount_split) beside its unsplit
twin and beside what a user had to do for the same per-class counts before it existed.  Prints one JSON line (recorded as
profiles/bincount_split_bench.json).

    python scripts/bincount_split_bench.py [--rounds 5] [--shapes small,big] [--out FILE]

Shapes and masks are those of scripts/exclude_bench.py: "small" = 4096 x 4096 drugs x 896 outcomes in bf16x3, "big" = 100 352 x
100 352 x 64 in f16; masks (symmetric, pipeline.known_pairs_mask, built outside the timed region): empty (a shared plane without
a bit: what the mask machinery itself costs), random1 (1 % of the pairs, uniform), hub1 (the same number of pairs, Zipf(1) hubs),
random1_per (small only: one plane per outcome).  Lower-triangle mode, 1000 edges per outcome.  Variants:
  screen_twin / histogram_twin        ops.bilinear_bincount without a mask: the unsplit sweep, the yardstick of every ratio -- edges
                                      at the pipeline.top_pairs(K = 1000) scores (nearly every score takes the two-compare fast path)
                                      and 1000 evenly spaced edges over the score range (every score is searched);
  screen_<mask> / histogram_<mask>    the same calls with split=<mask>;
  recovery_<mask>                     pipeline.recovery_at_cuts at the top_pairs(K = 1000) scores, end to end (sort, dedupe, sweep,
                                      cumsum, scatter, ratios);
  dense_bucketize / dense_bucketize_split   the route possible before: the dense head on blocks of head rows sized to an 8 GB buffer
                                      (2^31 scores), torch.searchsorted (right=True) + torch.bincount over every block, without and
                                      with the class bit of every entry (ops.pair_mask_rows of the random1 mask) folded into the bin
                                      index.  (It does not even mask the upper triangle.)
All variants run in one process, alternating round by round; a round times each variant over a window of at least --window seconds
of back-to-back calls with HIP events (the dense routes: one pass over all row blocks per round, --baseline-rounds rounds).  ms per
call: median [min, max] over the rounds."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from madrigal_amd import models as M, ops, pipeline  # noqa: E402
from exclude_bench import SHAPES, DecoderOnly, build_masks, mask_stats, window_ms  # noqa: E402

B = 1000


def bench_shape(name, N, L, prec, rounds, window_s, baseline_rounds):
    model = DecoderOnly(L, 0).cuda().eval()
    z = torch.randn(N, 128, generator=torch.Generator().manual_seed(1)).cuda()
    w = model.decoder.symmetric_weight()
    masks = build_masks(name, N, L)
    res = {"N": N, "L": L, "precision": prec, "edges": B, "masks": {k: mask_stats(m, N) for k, m in masks.items()}}
    old = M._state["precision"]
    M._state["precision"] = prec
    try:
        hits = pipeline.top_pairs(model, z, B)[0].contiguous()                     # [L, 1000] descending
        screen = torch.sort(hits, dim=1).values.contiguous()
        top = float(ops.bilinear_allpairs(z, z, w, precision=prec, epilogue=ops.EPI_ROWSTATS)[..., 1].max())
        even = torch.linspace(-top, top, B, device="cuda")[None, :].expand(L, -1).contiguous()
        block = max(1, min(N, (1 << 31) // (L * N)))      # 2^31 scores: torch.searchsorted cannot be launched over 2^32
        buf = torch.empty(L * block * N, dtype=torch.float32, device="cuda")
        offs = (torch.arange(L, device="cuda", dtype=torch.int32) * (2 * (B + 1)))[:, None]

        def dense(split):
            mask = masks["random1"]
            total = torch.zeros(L * 2 * (B + 1), dtype=torch.int64, device="cuda")
            for r0 in range(0, N, block):
                r1 = min(N, r0 + block)
                s = ops.bilinear_allpairs(z[r0:r1], z, w, precision=prec, out=buf.view(-1)[: L * (r1 - r0) * N].view(L, r1 - r0, N))
                idx = torch.searchsorted(screen, s.view(L, -1), right=True, out_int32=True)
                if split:
                    bit = ops.pair_mask_rows(mask, 0, torch.arange(r0, r1, device="cuda"), N).view(1, -1)
                    idx += bit.to(torch.int32) * (B + 1)
                total += torch.bincount((idx + offs).view(-1), minlength=L * 2 * (B + 1))
                del idx
            return total

        variants = {"screen_twin": lambda: ops.bilinear_bincount(z, z, w, screen, eligible="lower", precision=prec),
                    "histogram_twin": lambda: ops.bilinear_bincount(z, z, w, even, eligible="lower", precision=prec)}
        for key, m in masks.items():
            variants[f"screen_{key}"] = lambda m=m: ops.bilinear_bincount(z, z, w, screen, eligible="lower", precision=prec, split=m)
            variants[f"histogram_{key}"] = lambda m=m: ops.bilinear_bincount(z, z, w, even, eligible="lower", precision=prec, split=m)
            variants[f"recovery_{key}"] = lambda m=m: pipeline.recovery_at_cuts(model, z, m, hits)
        variants["dense_bucketize"] = lambda: dense(False)
        variants["dense_bucketize_split"] = lambda: dense(True)
        # what is being timed computes what it should: the classes add up to the twin, table 1 of the empty mask is empty
        for edges, twin in ((screen, "screen_twin"), (even, "histogram_twin")):
            ref = variants[twin]()
            for key, m in masks.items():
                got = ops.bilinear_bincount(z, z, w, edges, eligible="lower", precision=prec, split=m)
                assert torch.equal(got.sum(0), ref), (twin, key)
                assert key != "empty" or not bool(got[1].any())
        counts = ops.bilinear_bincount(z, z, w, screen, eligible="lower", precision=prec, split=masks["random1"])
        res["known_pairs_random1"] = int(counts[1, 0].sum())
        res["screen_fraction_of_scores_searched"] = float((counts[:, :, 1:-1].sum((0, 2)).double() / counts.sum((0, 2)).double()).mean())
        reps, times = {}, {v: [] for v in variants}
        for v, fn in variants.items():               # warm-up, and the number of calls that fills the window
            if v.startswith("dense"):
                if baseline_rounds:
                    fn()                             # one pass per window whatever it takes
                    torch.cuda.synchronize()
                    reps[v] = 1
                continue
            fn()
            torch.cuda.synchronize()
            reps[v] = max(1, math.ceil(window_s * 1e3 / max(window_ms(fn, 1), 1e-3)))
        for rnd in range(rounds):
            for v, fn in variants.items():
                if v.startswith("dense") and rnd >= baseline_rounds:
                    continue
                times[v].append(window_ms(fn, reps[v]))
    finally:
        M._state["precision"] = old
    res["baseline_row_block"] = block
    res["calls_per_window"] = reps
    for v, ts in times.items():
        if ts:
            res[v] = {"ms": round(float(np.median(ts)), 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)], "rounds": len(ts)}
    for key in masks:
        res[f"screen_{key}_over_twin"] = round(res[f"screen_{key}"]["ms"] / res["screen_twin"]["ms"], 3)
        res[f"histogram_{key}_over_twin"] = round(res[f"histogram_{key}"]["ms"] / res["histogram_twin"]["ms"], 3)
        res[f"recovery_{key}_over_screen_twin"] = round(res[f"recovery_{key}"]["ms"] / res["screen_twin"]["ms"], 3)
    if "dense_bucketize_split" in res:
        res["dense_bucketize_split_over_screen_random1"] = round(res["dense_bucketize_split"]["ms"] / res["screen_random1"]["ms"], 2)
        res["dense_bucketize_over_screen_twin"] = round(res["dense_bucketize"]["ms"] / res["screen_twin"]["ms"], 2)
    del masks, buf
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--baseline-rounds", type=int, default=1, help="rounds that also run the dense routes (tens of seconds at the big shape)")
    ap.add_argument("--window", type=float, default=0.4, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--shapes", default="small,big")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bincount_split_bench needs a GPU"
    res = {"metric": "bilinear_bincount_split_over_twin", "unit": "ratio", "higher_is_better": False}
    for name in a.shapes.split(","):
        N, L, prec = SHAPES[name]
        res[name] = bench_shape(name, N, L, prec, a.rounds, a.window, a.baseline_rounds)
        print(f"# {name}: " + json.dumps(res[name]), file=sys.stderr, flush=True)
    res["value"] = res[a.shapes.split(",")[0]]["screen_empty_over_twin"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
