#!/usr/bin/env python3
"""Time the known-pair exclusion masks of the in-sweep screening products (csrc/pairmask.hip, the MASKED instantiations of
csrc/topk.hip and csrc/select.hip) beside the unmasked kernels.  Prints one JSON line (recorded as profiles/exclude_bench.json).

    python scripts/exclude_bench.py [--rounds 5] [--shapes small,big] [--out FILE]

Shapes: "small" = 4096 x 4096 drugs x 896 outcomes in bf16x3 (BASELINE configs[1]); "big" = 100 352 x 100 352 x 64 in f16
(BASELINE configs[4] with 64 of its 1 024 outcomes).  Masks (all symmetric, built by pipeline.known_pairs_mask, outside the timed
region; "bits" is what they hold):
  empty       a shared plane without a bit: what the mask machinery itself costs;
  random1     a shared plane with 1 % of the pairs set, uniformly;
  hub1        a shared plane with the same number of listed pairs whose first drug is drawn with Zipf(1) probabilities over the
              drugs -- a few hubs with thousands of known partners, most drugs with a handful -- and a uniform partner;
  random1_per (small only) one plane per outcome, each with its own 1 %.
Variants:
  topk_unmasked / topk_<mask>            ops.bilinear_topk, k = 16, not_self -- the sweep of pipeline.top_partners;
  pairs_unmasked_<mask> / pairs_<mask>   pipeline.pairs_above end to end (count, cumsum, host read, allocation, fill, head expansion)
                                         without and with exclude=, both at the cut of the 1000th best NOVEL pair of every
                                         outcome (top_pairs(K = 1000, exclude=mask)): the unmasked call also returns, and pays for, the
                                         known pairs above that cut.
All variants run in one process, alternating round by round; a round times each variant over a window of at least --window seconds
of back-to-back calls with HIP events.  ms per call: median [min, max] over the rounds."""
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


def pair_lists(N, n_pairs, kind, gen):
    """(heads, tails) int64 on the GPU: n_pairs listed pairs, i != j."""
    if kind == "random":
        h = torch.randint(0, N, (n_pairs,), device="cuda", generator=gen)
    else:                                                         # Zipf(1) over a random order of the drugs, by inverse CDF
        cdf = torch.cumsum(1.0 / torch.arange(1, N + 1, device="cuda", dtype=torch.float64), 0)
        u = torch.rand(n_pairs, device="cuda", generator=gen, dtype=torch.float64) * cdf[-1]
        h = torch.randperm(N, device="cuda", generator=gen)[torch.searchsorted(cdf, u).clamp(max=N - 1)]
    t = torch.randint(0, N - 1, (n_pairs,), device="cuda", generator=gen)
    return h, t + (t >= h)


def build_masks(name, N, L):
    gen = torch.Generator(device="cuda").manual_seed(7)
    n_pairs = round(0.01 * N * N / 2)                             # symmetric: two bits per listed pair
    masks = {"empty": pipeline.known_pairs_mask(N, [], [])}
    for kind, key in (("random", "random1"), ("zipf", "hub1")):
        h, t = pair_lists(N, n_pairs, kind, gen)
        masks[key] = pipeline.known_pairs_mask(N, h, t)
        del h, t
    if name == "small":
        planes = []
        for l0 in range(0, L, 64):                               # per-outcome planes, 64 outcomes' lists at a time
            l1 = min(L, l0 + 64)
            h, t = pair_lists(N, n_pairs * (l1 - l0), "random", gen)
            lab = torch.arange(l1 - l0, device="cuda").repeat_interleave(n_pairs)
            planes.append(pipeline.known_pairs_mask(N, h, t, labels=lab, n_labels=l1 - l0))
            del h, t, lab
        masks["random1_per"] = torch.cat(planes)
    return masks


def mask_stats(mask, N):
    """Bits set and the largest number of excluded partners of one drug (first plane)."""
    bits = 0
    for p in range(mask.shape[0]):
        w = mask[p].view(-1)
        for s in range(0, w.numel(), 1 << 26):
            c = w[s:s + (1 << 26)].to(torch.int64) & 0xFFFFFFFF
            c = c - ((c >> 1) & 0x55555555)
            c = (c & 0x33333333) + ((c >> 2) & 0x33333333)
            c = (c + (c >> 4)) & 0x0F0F0F0F
            bits += int(((c * 0x01010101) >> 24 & 0xFF).sum())
    col_deg = (mask[0, :, :N] != 0).sum(0)                       # a lower bound per column; symmetric masks: per drug
    top = int(torch.argmax(col_deg))
    deg = int(ops.pair_mask_rows(mask, 0, torch.tensor([top], device="cuda"), N).sum())
    return {"planes": int(mask.shape[0]), "bits": bits, "fraction_of_pairs": round(bits / (mask.shape[0] * N * N), 5), "largest_degree": deg}


def bench_shape(name, N, L, prec, rounds, window_s):
    model = DecoderOnly(L, 0).cuda().eval()
    z = torch.randn(N, 128, generator=torch.Generator().manual_seed(1)).cuda()
    w = model.decoder.symmetric_weight()
    masks = build_masks(name, N, L)
    res = {"N": N, "L": L, "precision": prec, "masks": {k: mask_stats(m, N) for k, m in masks.items()}}
    old = M._state["precision"]
    M._state["precision"] = prec
    try:
        variants = {"topk_unmasked": lambda: ops.bilinear_topk(z, z, w, 16, eligible="not_self", precision=prec)}
        selected = {}
        for key, m in masks.items():
            variants[f"topk_{key}"] = lambda m=m: ops.bilinear_topk(z, z, w, 16, eligible="not_self", precision=prec, exclude=m)
            cut = pipeline.top_pairs(model, z, 1000, exclude=m)[0][:, -1].contiguous()
            variants[f"pairs_unmasked_{key}"] = lambda cut=cut: pipeline.pairs_above(model, z, cut, max_bytes=1 << 40)
            variants[f"pairs_{key}"] = lambda cut=cut, m=m: pipeline.pairs_above(model, z, cut, max_bytes=1 << 40, exclude=m)
            selected[key] = {"unmasked": int(variants[f"pairs_unmasked_{key}"]()[1].numel()), "masked": int(variants[f"pairs_{key}"]()[1].numel())}
        reps, times = {}, {v: [] for v in variants}
        for v, fn in variants.items():               # warm-up, and the number of calls that fills the window
            fn()
            torch.cuda.synchronize()
            reps[v] = max(1, math.ceil(window_s * 1e3 / max(window_ms(fn, 1), 1e-3)))
        for _ in range(rounds):
            for v, fn in variants.items():
                times[v].append(window_ms(fn, reps[v]))
    finally:
        M._state["precision"] = old
    res["calls_per_window"] = reps
    res["selected_pairs"] = selected
    for v, ts in times.items():
        res[v] = {"ms": round(float(np.median(ts)), 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)], "rounds": len(ts)}
    for key in masks:
        res[f"topk_{key}_over_unmasked"] = round(res[f"topk_{key}"]["ms"] / res["topk_unmasked"]["ms"], 3)
        res[f"pairs_{key}_over_unmasked"] = round(res[f"pairs_{key}"]["ms"] / res[f"pairs_unmasked_{key}"]["ms"], 3)
    del masks
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--shapes", default="small,big")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "exclude_bench needs a GPU"
    res = {"metric": "bilinear_topk_masked_over_unmasked", "unit": "ratio", "higher_is_better": False}
    for name in a.shapes.split(","):
        N, L, prec = SHAPES[name]
        res[name] = bench_shape(name, N, L, prec, a.rounds, a.window)
        print(f"# {name}: " + json.dumps(res[name]), file=sys.stderr, flush=True)
    res["value"] = res[a.shapes.split(",")[0]]["topk_empty_over_unmasked"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
