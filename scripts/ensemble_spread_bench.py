#!/usr/bin/env python3
"""Time the checkpoint-ensemble spread (csrc/ensemble_spread.hip: mdg_bilinear_ensemble_spread, mdg_bilinear_ensemble_spread_topk)
against the mean-only screen it was built from and against what was possible before it existed.  Prints one JSON line (recorded as
profiles/ensemble_spread_bench.json) and, on stderr, the table of README.md with every shape that loses to the old route in bold.

    python scripts/ensemble_spread_bench.py [--rounds 3] [--Ks 2,5] [--out FILE]

4096 x 4096 drugs x 896 outcomes, bf16x3, k = 16, not_self, kappa = -1.  Embeddings are N(0,1) * 0.3 and W ~ N(0,1) / sqrt(128),
symmetrised: logits of a few units, no saturated probabilities, so the lists keep changing through the whole sweep.  Per K:
  spread_topk_k16    ops.bilinear_ensemble_spread_topk
  ens_topk_k16       ops.bilinear_ensemble_topk at the same K and k: the difference is the price of the second moment, the payloads
                     and the narrower chunk (T is rebuilt every 2 tiles instead of every 6)
  old_topk_k16       what was possible before: K single-model ops.bilinear_ensemble_sigmoid([m]) calls over blocks of head rows
                     sized so that the K tensors fill 3 GiB, torch.mean + torch.std(unbiased=False) over the stack, kappa * std +
                     mean, torch.topk(16) over every block (it does not even mask the drug itself)
  spread_dense_L{Ld} ops.bilinear_ensemble_spread(kappa = -1) over the first Ld outcomes (mean, std and bound: 3 x Ld x N x N x 4 B)
  ens_dense_L{Ld}    ops.bilinear_ensemble_sigmoid over the same outcomes, general sweep (cloned tails): the mean alone, the price
                     list's other end for the dense kernel.  (A torch-route baseline for the three dense tensors -- K single-model
                     tensors, torch.mean / torch.std / torch.add into preallocated slices -- is not part of this script: DESIGN.md
                     4am.)
All variants run in one process, alternating round by round; a round times each variant over a window of at least --window seconds
of back-to-back calls with HIP events (the old routes: one pass).  ms per call: median [min, max] over the rounds.  Every warm-up
and every timed window is reported on stderr as it ends."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from madrigal_amd import ops  # noqa: E402

PREC = "bf16x3"
N, L, LD, TOPK, KAPPA = 4096, 896, 32, 16, -1.0
STACK_ELEMS = 3 << 28          # fp32 elements of the old route's stack of K per-model tensors (3 GiB)


def say(msg):
    print("# " + msg, file=sys.stderr, flush=True)


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def bench(Ks, rounds, window_s):
    Kmax = max(Ks)
    zs = [(torch.randn(N, 128, generator=torch.Generator().manual_seed(10 + m)) * 0.3).cuda() for m in range(Kmax)]
    ws = [ops.symmetrize((torch.randn(L, 128, 128, generator=torch.Generator().manual_seed(50 + m)) / 128 ** 0.5).cuda()) for m in range(Kmax)]
    wd = [w[:LD] for w in ws]
    spread_out = tuple(ops.empty_scores(LD, N, N, "cuda") for _ in range(3))
    blocks = {K: max(1, min(N, STACK_ELEMS // (K * L * N))) for K in Ks}          # head rows per block of the old top-k route
    stack = torch.empty(STACK_ELEMS, dtype=torch.float32, device="cuda")
    ens_out = ops.empty_scores(LD, N, N, "cuda")
    tails = [z.clone() for z in zs]                # another object on the tail side: the general sweep, as the spread runs

    def old_topk(K):
        block = blocks[K]

        def run():
            for r0 in range(0, N, block):
                r1 = min(N, r0 + block)
                p = stack[: K * L * (r1 - r0) * N].view(K, L, r1 - r0, N)
                for m in range(K):
                    ops.bilinear_ensemble_sigmoid([zs[m][r0:r1]], [zs[m]], [ws[m]], precision=PREC, out=p[m])
                bound = torch.add(p.mean(0), p.std(0, unbiased=False), alpha=KAPPA)
                torch.topk(bound, TOPK, dim=2)
        return run

    variants = {}
    for K in Ks:
        variants[f"K{K}_spread_topk_k{TOPK}"] = lambda K=K: ops.bilinear_ensemble_spread_topk(zs[:K], zs[:K], ws[:K], TOPK, KAPPA,
                                                                                             eligible="not_self", precision=PREC)
        variants[f"K{K}_ens_topk_k{TOPK}"] = lambda K=K: ops.bilinear_ensemble_topk(zs[:K], zs[:K], ws[:K], TOPK, eligible="not_self", precision=PREC)
        variants[f"K{K}_old_topk_k{TOPK}"] = old_topk(K)
        variants[f"K{K}_spread_dense_L{LD}"] = lambda K=K: ops.bilinear_ensemble_spread(zs[:K], zs[:K], wd[:K], kappa=KAPPA, precision=PREC,
                                                                                       out=spread_out)
        variants[f"K{K}_ens_dense_L{LD}"] = lambda K=K: ops.bilinear_ensemble_sigmoid(zs[:K], tails[:K], wd[:K], precision=PREC, out=ens_out)
    slow = lambda nm: "_old_" in nm      # noqa: E731
    reps, times = {}, {nm: [] for nm in variants}
    for nm, fn in variants.items():               # warm-up, and the number of calls that fills the window
        say(f"warm-up {nm} ...")
        fn()
        torch.cuda.synchronize()
        one = window_ms(fn, 1)
        reps[nm] = 1 if slow(nm) else max(1, math.ceil(window_s * 1e3 / max(one, 1e-3)))
        say(f"warm-up {nm}: {one:.2f} ms, {reps[nm]} call(s) per window")
    for rnd in range(rounds):
        for nm, fn in variants.items():
            times[nm].append(window_ms(fn, reps[nm]))
            say(f"round {rnd} {nm}: {times[nm][-1]:.2f} ms")
    res = {"N": N, "L": L, "L_dense": LD, "k": TOPK, "kappa": KAPPA, "eligible": "not_self", "precision": PREC, "z_scale": 0.3,
           "chunk_tiles": ops.bilinear_ensemble_spread_chunk_tiles(), "mean_only_chunk_tiles": ops.bilinear_ensemble_topk_chunk_tiles(),
           "old_route_stack_bytes": 4 * STACK_ELEMS, "old_topk_row_block": blocks, "calls_per_window": reps}
    for nm, ts in times.items():
        res[nm] = {"ms": round(float(np.median(ts)), 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)], "rounds": len(ts)}
    ms = lambda nm: res[nm]["ms"]      # noqa: E731
    for K in Ks:
        res[f"K{K}_spread_topk_over_ens_topk"] = round(ms(f"K{K}_spread_topk_k{TOPK}") / ms(f"K{K}_ens_topk_k{TOPK}"), 3)
        res[f"K{K}_old_topk_over_spread_topk"] = round(ms(f"K{K}_old_topk_k{TOPK}") / ms(f"K{K}_spread_topk_k{TOPK}"), 2)
        res[f"K{K}_spread_dense_over_ens_dense"] = round(ms(f"K{K}_spread_dense_L{LD}") / ms(f"K{K}_ens_dense_L{LD}"), 3)
    return res


def table(res, Ks):
    """README.md's rows; a product that is slower than the old route is printed in bold."""
    bold = lambda new, old, s: f"**{s}**" if new > old else s      # noqa: E731
    rows = ["| K | product | this | mean-only product | old route | old / this |", "|---|---|---|---|---|---|"]
    for K in Ks:
        t, e, o = (res[f"K{K}_{v}_k{TOPK}"]["ms"] for v in ("spread_topk", "ens_topk", "old_topk"))
        rows.append(f"| {K} | " + bold(t, o, f"top-k by the bound, k = {TOPK}, {L} outcomes") + f" | {t:.1f} ms | {e:.1f} ms | {o:.1f} ms | "
                    + bold(t, o, f"{o / t:.2f}x") + " |")
        d, e = res[f"K{K}_spread_dense_L{LD}"]["ms"], res[f"K{K}_ens_dense_L{LD}"]["ms"]
        rows.append(f"| {K} | mean + std + bound dense, {LD} outcomes | {d:.2f} ms | {e:.2f} ms | | |")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.4, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--Ks", default="2,5")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ensemble_spread_bench needs a GPU"
    Ks = tuple(int(x) for x in a.Ks.split(","))
    res = {"metric": "bilinear_ensemble_spread_topk_ms", "unit": "ms", "higher_is_better": False, "device": torch.cuda.get_device_name(0)}
    res.update(bench(Ks, a.rounds, a.window))
    res["value"] = res[f"K{max(Ks)}_spread_topk_k{TOPK}"]["ms"]
    print(table(res, Ks), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
