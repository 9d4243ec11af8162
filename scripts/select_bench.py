#!/usr/bin/env python3
"""Time the threshold-selecting epilogue of the all-pairs head (csrc/select.hip, mdg_bilinear_select_count / _fill) against the
bare sweep and against the only route that existed before it.  Prints one JSON line (recorded as profiles/select_bench.json).

    python scripts/select_bench.py [--rounds 5] [--shapes small,big] [--out FILE]

Shapes: "small" = 4096 x 4096 drugs x 896 outcomes in bf16x3 (BASELINE configs[1]); "big" = 100 352 x 100 352 x 64 in f16
(BASELINE configs[4] with 64 of its 1 024 outcomes: the cost per outcome is what is reported).  Everything selects in `lower`
mode (the unordered pairs i > j).  Cuts, per outcome, computed outside the timed region:
  K1000   the 1000th value of pipeline.top_pairs(K = 1000): about 1000 pairs per outcome;
  p01     (small only) the value with 1 % of the outcome's lower-triangle scores at or above it (from the dense general sweep,
          scored once in outcome chunks): about 84 000 pairs per outcome.
Variants, per shape:
  rowstats            ops.bilinear_allpairs(..., EPI_ROWSTATS): the bare row-statistics sweep (all N x N scores; it has no `lower` mode)
  count_none          ops.bilinear_select_count at +inf: the bare `lower` sweep -- pass-through only, nothing selected
  count_<cut>         ops.bilinear_select_count
  fill_<cut>          mdg_bilinear_select_fill alone, into preallocated outputs with the row pointers of the count
  pairs_above_<cut>   pipeline.pairs_above end to end (count, cumsum, host read, allocation, fill, head expansion)
  dense_nonzero_<cut> the route that existed before: the dense head on blocks of head rows sized to a 16 GB buffer (what
                      pipeline.score_all_pairs(head_rows=...) launches), (S >= cut) & (j < i), torch.nonzero and the selected values
                      of every block (in outcome slices of fewer than 2^31 scores, torch.nonzero's limit) -- every score goes to HBM
                      and comes back.
All variants run in one process, alternating round by round; a round times each variant over a window of at least --window
seconds of back-to-back calls with HIP events (the dense route: one pass over all row blocks per round).  ms per call: median
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
from madrigal_amd._lib import call  # noqa: E402

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


def quantile_cuts(model, z, L, top_fraction, chunk=16):
    """Per outcome the value with `top_fraction` of the strict-lower-triangle scores of the dense general sweep at or above it."""
    N = z.shape[0]
    ii, jj = torch.tril_indices(N, N, -1, device=z.device)
    n_pairs = ii.numel()
    k = n_pairs - max(1, round(top_fraction * n_pairs)) + 1          # 1-based place in ascending order
    cuts = torch.empty(L, dtype=torch.float32, device=z.device)
    zc = z.clone()
    with torch.no_grad():
        for s in range(0, L, chunk):
            e = min(L, s + chunk)
            dense = model.decoder(zc, z, (s, e))
            cuts[s:e] = torch.kthvalue(dense[:, ii, jj], k, dim=1).values
            del dense
    return cuts


def bench_shape(name, N, L, prec, rounds, window_s, baseline_rounds):
    model = DecoderOnly(L, 0).cuda().eval()
    z = torch.randn(N, 128, generator=torch.Generator().manual_seed(1)).cuda()
    w = model.decoder.symmetric_weight()
    block = max(1, min(N, (16 << 30) // (L * N * 4)))
    buf = torch.empty(L * block * N, dtype=torch.float32, device="cuda")
    cols_of = torch.arange(N, device="cuda")[None, None, :]
    old = M._state["precision"]
    M._state["precision"] = prec          # the decoder's precision (set_precision covers the whole-model modes; the head also runs "f16")
    try:
        cuts = {"K1000": pipeline.top_pairs(model, z, 1000)[0][:, -1].contiguous()}
        if name == "small":
            cuts["p01"] = quantile_cuts(model, z, L, 0.01)
        variants = {
            "rowstats": lambda: ops.bilinear_allpairs(z, z, w, precision=prec, epilogue=ops.EPI_ROWSTATS),
            "count_none": lambda thr=torch.full((L,), float("inf"), device="cuda"): ops.bilinear_select_count(z, z, w, thr, eligible="lower", precision=prec),
        }
        selected, keep = {}, []
        for cut, thr in cuts.items():
            row_ptr, cols, vals = ops.bilinear_select(z, z, w, thr, eligible="lower", precision=prec, max_bytes=1 << 40)
            selected[cut] = int(cols.numel())
            keep.append((row_ptr, cols, vals))
            ws, nbytes = ops._scratch("mdg_bilinear_select_workspace_bytes", z.device, N, N, L, 128, ops.HEAD_PRECISIONS[prec])

            def fill(thr=thr, row_ptr=row_ptr, cols=cols, vals=vals, ws=ws, nbytes=nbytes):
                call("mdg_bilinear_select_fill", z.data_ptr(), z.data_ptr(), w.data_ptr(), thr.data_ptr(), row_ptr.data_ptr(), cols.data_ptr(),
                     vals.data_ptr(), N, N, L, 128, ops.HEAD_PRECISIONS[prec], ops.TOPK_ELIGIBLE["lower"], ops._ptr(ws), nbytes, ops._stream(z))

            def dense_route(thr=thr):
                found = 0
                for r0 in range(0, N, block):
                    r1 = min(N, r0 + block)
                    s = ops.bilinear_allpairs(z[r0:r1], z, w, precision=prec, out=buf.view(-1)[: L * (r1 - r0) * N].view(L, r1 - r0, N))
                    below = cols_of < torch.arange(r0, r1, device="cuda")[None, :, None]
                    lc = max(1, (2 ** 31 - 1) // ((r1 - r0) * N))               # torch.nonzero takes fewer than 2^31 elements at a time
                    for l0 in range(0, L, lc):
                        sl = s[l0:l0 + lc]
                        m = (sl >= thr[l0:l0 + lc, None, None]) & below
                        nz = m.nonzero()
                        found += nz.shape[0] + sl[m].numel()
                return found

            variants[f"count_{cut}"] = lambda thr=thr: ops.bilinear_select_count(z, z, w, thr, eligible="lower", precision=prec)
            variants[f"fill_{cut}"] = fill
            variants[f"pairs_above_{cut}"] = lambda thr=thr: pipeline.pairs_above(model, z, thr, max_bytes=1 << 40)
            variants[f"dense_nonzero_{cut}"] = dense_route
        reps, times = {}, {v: [] for v in variants}
        for v, fn in variants.items():               # warm-up, and the number of calls that fills the window
            fn()
            torch.cuda.synchronize()
            one = window_ms(fn, 1)
            reps[v] = 1 if v.startswith("dense_nonzero") else max(1, math.ceil(window_s * 1e3 / max(one, 1e-3)))
        for rnd in range(rounds):
            for v, fn in variants.items():
                if v.startswith("dense_nonzero") and rnd >= baseline_rounds:
                    continue
                times[v].append(window_ms(fn, reps[v]))
    finally:
        M._state["precision"] = old
    res = {"N": N, "L": L, "precision": prec, "eligible": "lower", "baseline_row_block": block, "calls_per_window": reps,
           "selected_pairs": selected}
    for v, ts in times.items():
        res[v] = {"ms": round(float(np.median(ts)), 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)],
                  "ms_per_outcome": round(float(np.median(ts)) / L, 4), "rounds": len(ts)}
    ms = lambda v: res[v]["ms"]  # noqa: E731
    res["count_none_over_rowstats"] = round(ms("count_none") / ms("rowstats"), 3)
    for cut in cuts:
        res[f"count_{cut}_over_count_none"] = round(ms(f"count_{cut}") / ms("count_none"), 3)
        res[f"fill_{cut}_over_count_none"] = round(ms(f"fill_{cut}") / ms("count_none"), 3)
        res[f"dense_nonzero_{cut}_over_pairs_above_{cut}"] = round(ms(f"dense_nonzero_{cut}") / ms(f"pairs_above_{cut}"), 2)
    del buf, keep
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--baseline-rounds", type=int, default=2, help="rounds that also run the dense route (several seconds at the big shape)")
    ap.add_argument("--window", type=float, default=0.4, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--shapes", default="small,big")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "select_bench needs a GPU"
    res = {"metric": "bilinear_select_ms", "unit": "ms", "higher_is_better": False}
    for name in a.shapes.split(","):
        N, L, prec = SHAPES[name]
        res[name] = bench_shape(name, N, L, prec, a.rounds, a.window, a.baseline_rounds)
        print(f"# {name}: " + json.dumps(res[name]), file=sys.stderr, flush=True)
    first = a.shapes.split(",")[0]
    res["value"] = res[first]["pairs_above_K1000"]["ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
