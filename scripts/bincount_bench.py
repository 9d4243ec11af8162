#!/usr/bin/env python3
"""Time the counting epilogue of the all-pairs head (csrc/bincount.hip, mdg_bilinear_bincount) against the bare row-statistics
sweep and against what a user had to do for the same counts before it existed.  Prints one JSON line (recorded as
profiles/bincount_bench.json).

    python scripts/bincount_bench.py [--rounds 5] [--shapes small,big] [--out FILE]

Shapes: "small" = 4096 x 4096 drugs x 896 outcomes in bf16x3 (BASELINE configs[1]); "big" = 100 352 x 100 352 x 64 in f16
(BASELINE configs[4] with 64 of its 1 024 outcomes: the cost per outcome is what is reported).  Lower-triangle mode.  Variants:
  rowstats         (a) ops.bilinear_allpairs(..., EPI_ROWSTATS): the bare sweep (all tiles; the lower-triangle modes visit half)
  lower_k16        (b) ops.bilinear_topk(16, "lower"): the other reducing epilogue over the same tiles, for scale
  screen_1000      (c) ops.bilinear_bincount with 1000 edges per outcome at the pipeline.top_pairs(K = 1000) scores: ranks of
                       screened hits, nearly every score takes the two-compare fast path
  histogram_1000   (d) ops.bilinear_bincount with 1000 evenly spaced edges over the score range: every score is searched
  ranks_of_hits    (e) pipeline.normalized_ranks_of(top_pairs values), end to end (sort, dedupe, sweep, cumsum, scatter)
  dense_bucketize  (f) the baseline: the dense head on blocks of head rows sized to an 8 GB buffer (2^31 scores) and torch.searchsorted
                       (right=True, the batched bucketize) + torch.bincount over every block -- every score goes to HBM and comes
                       back.  (It does not even mask the upper triangle.)
All variants run in one process, alternating round by round; a round times each variant over a window of at least --window
seconds of back-to-back calls with HIP events (the baseline: one pass over all row blocks per round).  ms per call: median
[min, max] over the rounds."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from madrigal_amd import models as M, ops, pipeline  # noqa: E402

SHAPES = {"small": (4096, 896, "bf16x3"), "big": (100_352, 64, "f16")}
B = 1000


class DecoderOnly(torch.nn.Module):
    def __init__(self, L, seed):
        super().__init__()
        self.decoder = M.BilinearDDIScorer(128, 128, L)
        torch.nn.utils.parametrize.register_parametrization(self.decoder, "weight", M.Symmetric())
        with torch.no_grad():
            self.decoder.parametrizations.weight.original.copy_(
                torch.randn(L, 128, 128, generator=torch.Generator().manual_seed(seed)) / 128 ** 0.5)


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def bench_shape(N, L, prec, rounds, window_s, baseline_rounds):
    model = DecoderOnly(L, 0).cuda().eval()
    z = torch.randn(N, 128, generator=torch.Generator().manual_seed(1)).cuda()
    w = model.decoder.symmetric_weight()
    old = M._state["precision"]
    M._state["precision"] = prec          # the decoder's precision (set_precision covers the whole-model modes; the head also runs "f16")
    try:
        hits = pipeline.top_pairs(model, z, B)[0]                                  # [L, 1000] descending
        screen = torch.sort(hits, dim=1).values.contiguous()
        top = float(ops.bilinear_allpairs(z, z, w, precision=prec, epilogue=ops.EPI_ROWSTATS)[..., 1].max())
        even = torch.linspace(-top, top, B, device="cuda")[None, :].expand(L, -1).contiguous()
        block = max(1, min(N, (1 << 31) // (L * N)))      # 2^31 scores: torch.searchsorted cannot be launched over 2^32
        buf = torch.empty(L * block * N, dtype=torch.float32, device="cuda")
        offs = (torch.arange(L, device="cuda", dtype=torch.int32) * (B + 1))[:, None]

        def baseline():
            total = torch.zeros(L * (B + 1), dtype=torch.int64, device="cuda")
            for r0 in range(0, N, block):
                r1 = min(N, r0 + block)
                s = ops.bilinear_allpairs(z[r0:r1], z, w, precision=prec, out=buf.view(-1)[: L * (r1 - r0) * N].view(L, r1 - r0, N))
                idx = torch.searchsorted(screen, s.view(L, -1), right=True, out_int32=True)
                total += torch.bincount((idx + offs).view(-1), minlength=L * (B + 1))
                del idx
            return total

        variants = {
            "rowstats": lambda: ops.bilinear_allpairs(z, z, w, precision=prec, epilogue=ops.EPI_ROWSTATS),
            "lower_k16": lambda: ops.bilinear_topk(z, z, w, 16, eligible="lower", precision=prec),
            "screen_1000": lambda: ops.bilinear_bincount(z, z, w, screen, eligible="lower", precision=prec),
            "histogram_1000": lambda: ops.bilinear_bincount(z, z, w, even, eligible="lower", precision=prec),
            "ranks_of_hits": lambda: pipeline.normalized_ranks_of(model, z, hits),
            "dense_bucketize": baseline,
        }
        reps, times = {}, {name: [] for name in variants}
        for name, fn in variants.items():               # warm-up, and the number of calls that fills the window
            if name == "dense_bucketize" and baseline_rounds == 0:
                continue
            fn()
            torch.cuda.synchronize()
            one = window_ms(fn, 1)
            reps[name] = 1 if name == "dense_bucketize" else max(1, math.ceil(window_s * 1e3 / max(one, 1e-3)))
        for rnd in range(rounds):
            for name, fn in variants.items():
                if name == "dense_bucketize" and rnd >= baseline_rounds:
                    continue
                times[name].append(window_ms(fn, reps[name]))
        counts = variants["screen_1000"]()
        inside = counts[:, 1:-1].sum(1).double() / counts.sum(1).double()
    finally:
        M._state["precision"] = old
    res = {"N": N, "L": L, "precision": prec, "edges": B, "baseline_row_block": block, "calls_per_window": reps,
           "screen_fraction_of_scores_searched": float(inside.mean())}
    for name, ts in times.items():
        if ts:
            res[name] = {"ms": round(float(np.median(ts)), 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)],
                         "ms_per_outcome": round(float(np.median(ts)) / L, 4), "rounds": len(ts)}
    ms = lambda name: res[name]["ms"]                                             # noqa: E731
    res["screen_over_rowstats"] = round(ms("screen_1000") / ms("rowstats"), 3)
    res["screen_over_lower_k16"] = round(ms("screen_1000") / ms("lower_k16"), 3)
    res["histogram_over_screen"] = round(ms("histogram_1000") / ms("screen_1000"), 3)
    res["histogram_over_rowstats"] = round(ms("histogram_1000") / ms("rowstats"), 3)
    if "dense_bucketize" in res:
        res["dense_bucketize_over_screen"] = round(ms("dense_bucketize") / ms("screen_1000"), 2)
    del buf
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--baseline-rounds", type=int, default=2, help="rounds that also run the dense baseline (tens of seconds at the big shape)")
    ap.add_argument("--window", type=float, default=0.4, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--shapes", default="small,big")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bincount_bench needs a GPU"
    res = {"metric": "bilinear_bincount_ms", "unit": "ms", "higher_is_better": False}
    for name in a.shapes.split(","):
        N, L, prec = SHAPES[name]
        res[name] = bench_shape(N, L, prec, a.rounds, a.window, a.baseline_rounds)
        print(f"# {name}: " + json.dumps(res[name]), file=sys.stderr, flush=True)
    first = a.shapes.split(",")[0]
    res["value"] = res[first]["screen_1000"]["ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
