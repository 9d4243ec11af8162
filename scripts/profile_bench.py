#!/usr/bin/env python3
"""Time the per-pair outcome profile of the all-pairs head (csrc/profile.hip, mdg_bilinear_profile) against the bare sweep and
against the only route that existed before it.  Prints one JSON line (recorded as profiles/profile_bench.json).

    python scripts/profile_bench.py [--rounds 5] [--shapes small,big] [--out FILE]

Shapes: "small" = 4096 x 4096 drugs x 896 outcomes in bf16x3 (BASELINE configs[1]); "big" = 100 352 x 100 352 x 64 in f16
(BASELINE configs[4] with 64 of its 1 024 outcomes).  Cuts: per outcome the 1000th value of pipeline.top_pairs(K = 1000), computed
outside the timed region; scales: a fixed positive vector.
Variants, per shape:
  rowstats          ops.bilinear_allpairs(..., EPI_ROWSTATS): the bare row-statistics sweep (all N x N scores of every outcome)
  profile_not_self  the profile of every ordered pair: small -- one ops.bilinear_profile call (three [N, N] results); big -- the three
  profile_lower     [N, N] results would be 121 GB, so the pass streams row blocks of --block rows into one reused triple, as
                    pipeline.most_flagged_pairs does: rows [r0, r1) against all drugs (not_self) or against the drugs [0, r1)
                    (lower: the rest of the block is the upper triangle), in "all" mode.  small/lower is one call in LOWER mode.
  dense_reduce      the route that existed before: the dense head on blocks of head rows sized to a 16 GB buffer (what
                    pipeline.score_all_pairs(head_rows=...) launches), then (S >= thr).sum(0), S.max(0) and S.argmax(0) in torch --
                    every score goes to HBM and comes back three times.  (It leaves the subtraction of the cuts and the scales
                    out, which a faithful margin would add as another pass.)
All variants run in one process, alternating round by round, timed with HIP events over a window of back-to-back calls (one pass
per round for the variants that take seconds).  ms per pass: median [min, max] over the rounds."""
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


def bench_shape(name, N, L, prec, rounds, window_s, baseline_rounds, block_rows):
    model = DecoderOnly(L, 0).cuda().eval()
    z = torch.randn(N, 128, generator=torch.Generator().manual_seed(1)).cuda()
    w = model.decoder.symmetric_weight()
    scale = (0.5 + torch.rand(L, generator=torch.Generator().manual_seed(2))).cuda()
    dense_block = max(1, min(N, (16 << 30) // (L * N * 4)))
    buf = torch.empty(L * dense_block * N, dtype=torch.float32, device="cuda")
    old = M._state["precision"]
    M._state["precision"] = prec
    try:
        thr = pipeline.top_pairs(model, z, 1000)[0][:, -1].contiguous()
        whole = 3 * 4 * N * N <= (8 << 30)                 # the three [N, N] results fit: one call; otherwise stream row blocks
        B = N if whole else block_rows
        out = ops._profile_out(None, B, N, z.device)
        flagged = {}

        def profile(mode):
            if whole:
                return ops.bilinear_profile(z, z, w, thr, scale=scale, eligible=mode, precision=prec, out=out)
            for r0 in range(0, N, B):
                r1 = min(N, r0 + B)
                nt = r1 if mode == "lower" else N
                o = tuple(t[: r1 - r0, :nt] for t in out)
                ops.bilinear_profile(z[r0:r1], z[:nt], w, thr, scale=scale, eligible="all", precision=prec, out=o)
            return out

        def dense_reduce():
            seen = 0
            for r0 in range(0, N, dense_block):
                r1 = min(N, r0 + dense_block)
                s = ops.bilinear_allpairs(z[r0:r1], z, w, precision=prec, out=buf[: L * (r1 - r0) * N].view(L, r1 - r0, N))
                count = (s >= thr[:, None, None]).sum(0)
                margin = s.max(0).values
                best = s.argmax(0)
                seen += count.numel() + margin.numel() + best.numel()
            return seen

        variants = {"rowstats": lambda: ops.bilinear_allpairs(z, z, w, precision=prec, epilogue=ops.EPI_ROWSTATS),
                    "profile_not_self": lambda: profile("not_self"), "profile_lower": lambda: profile("lower"), "dense_reduce": dense_reduce}
        reps, times = {}, {v: [] for v in variants}
        for v, fn in variants.items():               # warm-up, and the number of calls that fills the window
            fn()
            torch.cuda.synchronize()
            if v.startswith("profile") and whole:
                flagged[v] = int((out[0] > 0).sum())
            one = window_ms(fn, 1)
            reps[v] = 1 if v == "dense_reduce" else max(1, math.ceil(window_s * 1e3 / max(one, 1e-3)))
        for rnd in range(rounds):
            for v, fn in variants.items():
                if v == "dense_reduce" and rnd >= baseline_rounds:
                    continue
                times[v].append(window_ms(fn, reps[v]))
    finally:
        M._state["precision"] = old
    res = {"N": N, "L": L, "precision": prec, "profile_row_block": B, "dense_row_block": dense_block, "calls_per_window": reps,
           "pairs_flagged_at_least_once": flagged}
    for v, ts in times.items():
        res[v] = {"ms": round(float(np.median(ts)), 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)], "rounds": len(ts)}
    ms = lambda v: res[v]["ms"]  # noqa: E731
    for v in ("profile_not_self", "profile_lower"):
        res[f"{v}_over_rowstats"] = round(ms(v) / ms("rowstats"), 3)
        res[f"dense_reduce_over_{v}"] = round(ms("dense_reduce") / ms(v), 3)
    del buf, out
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--baseline-rounds", type=int, default=2, help="rounds that also run the dense route (seconds per pass)")
    ap.add_argument("--window", type=float, default=0.4, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--block", type=int, default=4096, help="head rows per call where the three [N, N] results do not fit")
    ap.add_argument("--shapes", default="small,big")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "profile_bench needs a GPU"
    res = {"metric": "bilinear_profile_ms", "unit": "ms", "higher_is_better": False}
    for name in a.shapes.split(","):
        N, L, prec = SHAPES[name]
        res[name] = bench_shape(name, N, L, prec, a.rounds, a.window, a.baseline_rounds, a.block)
        print(f"# {name}: " + json.dumps(res[name]), file=sys.stderr, flush=True)
    first = a.shapes.split(",")[0]
    res["value"] = res[first]["profile_not_self"]["ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
