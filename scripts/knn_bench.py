#!/usr/bin/env python3
"""Time the on-device k-nearest-neighbour sweep (csrc/knn.hip, ops.knn_topk) beside what was possible before it: row-blocked torch
normalise + matmul + topk on the GPU.  Prints one JSON line (recorded as profiles/knn_bench.json).

    python scripts/knn_bench.py [--rounds 5] [--shapes all,segmented,small] [--out profiles/knn_bench.json]

k = 20, cosine.  Shapes (queries x library, D = 128): "all" = 100 352 x 100 352 (every drug of BASELINE configs[4] against every
other); "segmented" = 4096 x 100 352 (32 row blocks: the column-segmented path); "small" = 2048 x 2048.  Variants, all in one
process, alternating round by round; a round times each variant over a window of at least --window seconds of back-to-back calls
with HIP events; ms per call: median [min, max] over the rounds:
  knn        ops.knn_topk (pre-pass, sweep, merge where segmented, and the host read of the status word);
  sweep      ops.knn_sweep_rowmax: the same pre-pass, sweep and host read with the list epilogue compiled out (a row maximum keeps
             the products live), the same segments, no merge;
  knn_alt    ops.knn_topk with another number of segments than the default: 4 where the default is 1 (the row blocks alone leave
             a partly filled last round of workgroups), 1 where it is more (what the segments buy);
  torch      the library normalised once per call, then per block of query rows (the largest whose fp32 similarity block stays under
             --block-bytes) normalise, ``@``, ``torch.topk``; the dense matrix of "all" would be 40 GB.
Derived: knn over sweep (the cost of the lists), torch over knn, and the share of the fp32 MFMA peak (157.3 TFLOP/s: 256 CUs x 4
SIMDs x 64 FLOP/clk x 2.4 GHz) of 2 nq nl 128 FLOP over the knn call and over the sweep call -- call times, not kernel times.  The
two routes' indices are compared once (rows whose k indices agree as sets): equal similarities aside, they differ where two
similarities lie within fp32 rounding of each other."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from madrigal_amd import ops  # noqa: E402

SHAPES = {"all": (100_352, 100_352), "segmented": (4096, 100_352), "small": (2048, 2048)}
K = 20
PEAK_F32_MFMA = 157.3e12


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def torch_route(q, lib, k, block_rows):
    ln = lib / torch.norm(lib, dim=1, keepdim=True)
    vals = torch.empty((q.shape[0], k), dtype=torch.float32, device=q.device)
    idx = torch.empty((q.shape[0], k), dtype=torch.int64, device=q.device)
    for r0 in range(0, q.shape[0], block_rows):
        blk = q[r0:r0 + block_rows]
        sim = (blk / torch.norm(blk, dim=1, keepdim=True)) @ ln.T
        v, i = sim.topk(k, dim=1, largest=True, sorted=True)
        vals[r0:r0 + block_rows], idx[r0:r0 + block_rows] = v, i
    return vals, idx


def bench_shape(nq, nl, rounds, window_s, block_bytes):
    gen = torch.Generator().manual_seed(nq + nl)
    lib = torch.randn(nl, 128, generator=gen).cuda()
    q = lib[:nq].contiguous() if nq <= nl else torch.randn(nq, 128, generator=gen).cuda()
    q = q + 0.5 * torch.randn(nq, 128, generator=gen).cuda()                  # every query has one clear neighbour and a noisy rest
    S = ops.knn_default_segments(nq, nl)
    block_rows = max(1, min(nq, block_bytes // (4 * nl)))
    alt = 4 if S == 1 else 1
    variants = {"knn": lambda: ops.knn_topk(q, lib, K),
                "sweep": lambda: ops.knn_sweep_rowmax(q, lib, segments=S),
                "knn_alt": lambda: ops.knn_topk(q, lib, K, segments=alt),
                "torch": lambda: torch_route(q, lib, K, block_rows)}
    res = {"nq": nq, "nl": nl, "k": K, "metric": "cosine", "segments": S, "alt_segments": alt, "torch_block_rows": block_rows}
    gi, ti = variants["knn"]()[1].long(), variants["torch"]()[1]
    res["rows_same_set"] = round(float((gi.sort(1)[0] == ti.sort(1)[0]).all(1).float().mean()), 6)
    res["rows_same_order"] = round(float((gi == ti).all(1).float().mean()), 6)
    del gi, ti
    reps, times = {}, {v: [] for v in variants}
    for v, fn in variants.items():                   # warm-up, and the number of calls that fills the window
        fn()
        torch.cuda.synchronize()
        reps[v] = max(1, math.ceil(window_s * 1e3 / max(window_ms(fn, 1), 1e-3)))
    for _ in range(rounds):
        for v, fn in variants.items():
            times[v].append(window_ms(fn, reps[v]))
    res["calls_per_window"] = reps
    for v, ts in times.items():
        res[v] = {"ms": round(float(np.median(ts)), 4), "ms_min_max": [round(min(ts), 4), round(max(ts), 4)], "rounds": len(ts)}
    flop = 2.0 * nq * nl * 128
    res["knn_over_sweep"] = round(res["knn"]["ms"] / res["sweep"]["ms"], 3)
    res["torch_over_knn"] = round(res["torch"]["ms"] / res["knn"]["ms"], 3)
    res["knn_alt_over_knn"] = round(res["knn_alt"]["ms"] / res["knn"]["ms"], 3)
    res["knn_fraction_of_f32_mfma_peak"] = round(flop / (res["knn"]["ms"] * 1e-3) / PEAK_F32_MFMA, 4)
    res["sweep_fraction_of_f32_mfma_peak"] = round(flop / (res["sweep"]["ms"] * 1e-3) / PEAK_F32_MFMA, 4)
    del q, lib
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--shapes", default="all,segmented,small")
    ap.add_argument("--block-bytes", type=int, default=1 << 30, help="largest fp32 similarity block of the torch route")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "knn_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "knn_bench needs a GPU"
    res = {"metric": "knn_topk_torch_over_knn", "unit": "ratio", "higher_is_better": True, "peak_f32_mfma_flops": PEAK_F32_MFMA}
    for name in a.shapes.split(","):
        res[name] = bench_shape(*SHAPES[name], a.rounds, a.window, a.block_bytes)
        print(f"# {name}: " + json.dumps(res[name]), file=sys.stderr, flush=True)
    res["value"] = res[a.shapes.split(",")[0]]["torch_over_knn"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
