#!/usr/bin/env python3
"""Time threshold selection over a checkpoint ensemble (csrc/ensemble_select.hip, mdg_bilinear_ensemble_select_count / _fill) against
what was possible before it existed and against the bare ensemble sweep.  Prints one JSON line (recorded as
profiles/ensemble_select_bench.json).

    python scripts/ensemble_select_bench.py [--rounds 3] [--shapes small,big] [--out FILE]

Shapes: "small" = 4096 x 4096 drugs x 896 outcomes, bf16x3, lower triangle, K in {1, 2, 5} checkpoints; "big" = 100 352 x 100 352
x 16, K = 5, cut (i) only (one outcome's [N,N] fp32 plane is 40 GB: the dense route exists only in row blocks).  Embeddings are
N(0,1) * 0.3 and W ~ N(0,1) / sqrt(128), symmetrised: logits of a few units, no saturated probabilities.  Two cuts per outcome:
  i    the probability of the 1000th best pair, from pipeline.ensemble_top_pairs(K = 1000): about 1000 pairs per outcome
  ii   the 0.99 quantile of the probabilities of a dense block of 64 head rows: about 1 % of the pairs
Variants per shape and K (T = selected pairs, recorded next to them):
  count_{cut}            ops.bilinear_ensemble_select_count, lower
  fill_{cut}             mdg_bilinear_ensemble_select_fill alone, into preallocated outputs with the row pointers of the count
  pairs_above_{cut}      pipeline.ensemble_pairs_above end to end: count, cumsum, the host read, fill, the head expansion
  topk1_lower            (b) ops.bilinear_ensemble_topk(k = 1, eligible="lower"): the nearest thing to the bare ensemble sweep
  dense_nonzero_{cut}    (a) what was possible before: ops.bilinear_ensemble_sigmoid over blocks of head rows sized to a 16 GB
                         buffer, then torch.nonzero of (P >= cut) & (j < i) and the value gather, block by block
  count_i_excl1pct       the count with an exclude= mask holding 1 % of all pairs (small shape, K = 5)
All variants run in one process, alternating round by round; a round times each variant over a window of at least --window
seconds of back-to-back calls with HIP events (the dense baseline: one pass over all row blocks).  ms per call: median [min, max]
over the rounds."""
import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from madrigal_amd import models as M, ops, pipeline  # noqa: E402
from madrigal_amd._lib import call  # noqa: E402

SHAPES = {"small": dict(N=4096, L=896, Ks=(1, 2, 5), cuts=("i", "ii")),
          "big": dict(N=100_352, L=16, Ks=(5,), cuts=("i",))}
PREC = "bf16x3"


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def c_fill(zs, ws, thr, row_ptr, cols, vals):
    """The fill pass alone through the C entry point (lower triangle, no mask)."""
    K, N, L = len(zs), zs[0].shape[0], ws[0].shape[0]
    buf, nbytes = ops._scratch("mdg_bilinear_ensemble_select_workspace_bytes", zs[0].device, N, N, L, 128, K, ops.ENSEMBLE_PRECISIONS[PREC])
    arr = lambda ts: (ctypes.c_void_p * K)(*[t.data_ptr() for t in ts])    # noqa: E731
    call("mdg_bilinear_ensemble_select_fill", arr(zs), arr(zs), arr(ws), K, thr.data_ptr(), row_ptr.data_ptr(), cols.data_ptr(), vals.data_ptr(),
         N, N, L, 128, ops.ENSEMBLE_PRECISIONS[PREC], ops.TOPK_ELIGIBLE["lower"], None if buf is None else buf.data_ptr(), nbytes,
         ops._stream(zs[0]), None, 0)


def bench_shape(name, N, L, Ks, cuts, rounds, window_s):
    Kmax = max(Ks)
    zs = [(torch.randn(N, 128, generator=torch.Generator().manual_seed(10 + m)) * 0.3).cuda() for m in range(Kmax)]
    raw = [(torch.randn(L, 128, 128, generator=torch.Generator().manual_seed(50 + m)) / 128 ** 0.5).cuda() for m in range(Kmax)]
    ws = [ops.symmetrize(w) for w in raw]
    block = max(1, min(N, (16 << 30) // (L * N * 4)))
    buf = torch.empty(L * block * N, dtype=torch.float32, device="cuda")
    col = torch.arange(N, device="cuda")[None, None, :]
    sub = max(1, ((1 << 31) - 1) // (L * N))

    def dense(K, thr, found):
        def run():
            n = 0
            for r0 in range(0, N, block):
                r1 = min(N, r0 + block)
                p = ops.bilinear_ensemble_sigmoid([z[r0:r1] for z in zs[:K]], zs[:K], ws[:K], precision=PREC,
                                                  out=buf[: L * (r1 - r0) * N].view(L, r1 - r0, N))
                for s0 in range(0, r1 - r0, sub):                  # torch.nonzero takes fewer than 2^31 elements per call
                    q = p[:, s0:s0 + sub]
                    hit = (q >= thr[:, None, None]) & (col < torch.arange(r0 + s0, r0 + s0 + q.shape[1], device="cuda")[None, :, None])
                    idx = torch.nonzero(hit)
                    v = q[idx[:, 0], idx[:, 1], idx[:, 2]]
                    n += int(v.numel())
            found[0] = n
        return run

    old = M._state["precision"]
    M._state["precision"] = PREC
    res = {"N": N, "L": L, "precision": PREC, "z_scale": 0.3, "eligible": "lower", "baseline_row_block": block}
    try:
        variants, slow, keep = {}, set(), []
        for K in Ks:
            thr = {}
            if "i" in cuts:
                thr["i"] = pipeline.ensemble_top_pairs(raw[:K], zs[:K], 1000)[0][:, -1].contiguous()
            if "ii" in cuts:
                rows = slice(N - 64, N)
                p = ops.bilinear_ensemble_sigmoid([z[rows] for z in zs[:K]], zs[:K], ws[:K], precision=PREC).reshape(L, -1)
                thr["ii"] = torch.sort(p, dim=1).values[:, int(0.99 * (p.shape[1] - 1))].contiguous()
                del p
            variants[f"K{K}_topk1_lower"] = lambda K=K: ops.bilinear_ensemble_topk(zs[:K], zs[:K], ws[:K], 1, eligible="lower", precision=PREC)
            for cut, t in thr.items():
                row_ptr, cols, vals = ops.bilinear_ensemble_select(zs[:K], zs[:K], ws[:K], t, eligible="lower", precision=PREC, max_bytes=1 << 40)
                T = int(cols.numel())
                res[f"K{K}_T_{cut}"] = T
                res[f"K{K}_selected_fraction_{cut}"] = T / (L * N * (N - 1) / 2)
                keep.append((row_ptr, cols, vals))
                variants[f"K{K}_count_{cut}"] = lambda K=K, t=t: ops.bilinear_ensemble_select_count(zs[:K], zs[:K], ws[:K], t, eligible="lower",
                                                                                                  precision=PREC)
                variants[f"K{K}_fill_{cut}"] = lambda K=K, t=t, o=(row_ptr, cols, vals): c_fill(zs[:K], ws[:K], t, *o)
                variants[f"K{K}_pairs_above_{cut}"] = lambda K=K, t=t: pipeline.ensemble_pairs_above(raw[:K], zs[:K], t, max_bytes=1 << 40)
                found = [None]
                variants[f"K{K}_dense_nonzero_{cut}"] = dense(K, t, found)
                slow.add(f"K{K}_dense_nonzero_{cut}")
                variants[f"K{K}_dense_nonzero_{cut}"]()
                res[f"K{K}_dense_nonzero_{cut}_agrees"] = found[0] == T
            if K == Kmax and name == "small":
                g = torch.Generator().manual_seed(3)
                n = N * N // 100
                known = ops.pair_mask(torch.randint(0, N, (n,), generator=g), torch.randint(0, N, (n,), generator=g), N, symmetric=True,
                                      device="cuda")
                variants[f"K{K}_count_i_excl1pct"] = lambda K=K, t=thr["i"]: ops.bilinear_ensemble_select_count(
                    zs[:K], zs[:K], ws[:K], t, eligible="lower", precision=PREC, exclude=known)
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
        for cut in cuts:
            res[f"K{K}_count_{cut}_over_topk1"] = round(ms(f"K{K}_count_{cut}") / ms(f"K{K}_topk1_lower"), 3)
            res[f"K{K}_fill_{cut}_over_count_{cut}"] = round(ms(f"K{K}_fill_{cut}") / ms(f"K{K}_count_{cut}"), 3)
            res[f"K{K}_dense_nonzero_{cut}_over_pairs_above_{cut}"] = round(ms(f"K{K}_dense_nonzero_{cut}") / ms(f"K{K}_pairs_above_{cut}"), 2)
    if f"K{Kmax}_count_i_excl1pct" in res:
        res[f"K{Kmax}_count_i_excl1pct_over_count_i"] = round(ms(f"K{Kmax}_count_i_excl1pct") / ms(f"K{Kmax}_count_i"), 3)
    del buf, keep
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.4, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--shapes", default="small,big")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ensemble_select_bench needs a GPU"
    res = {"metric": "bilinear_ensemble_select_ms", "unit": "ms", "higher_is_better": False, "device": torch.cuda.get_device_name(0)}
    for name in a.shapes.split(","):
        res[name] = bench_shape(name, rounds=a.rounds, window_s=a.window, **SHAPES[name])
        print(f"# {name}: " + json.dumps(res[name]), file=sys.stderr, flush=True)
    first = a.shapes.split(",")[0]
    res["value"] = res[first]["K5_pairs_above_i"]["ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
