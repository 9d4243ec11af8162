#!/usr/bin/env python3
"""Time the 16-bit destinations of the checkpoint-ensemble sweep (csrc/ensemble_store16.hip, mdg_bilinear_ensemble_sigmoid16)
against the fp32 product and against the only route to a 16-bit tensor that existed before it (the fp32 product + a cast).  Prints
one JSON line (recorded as profiles/ensemble_store16_bench.json).

    python scripts/ensemble_store16_bench.py [--rounds 5] [--Ks 1,2,5] [--out FILE]

At 4096 x 4096 drugs x 896 outcomes, bf16x3, K in {1, 2, 5} checkpoints, the symmetric sweep (z_tails[k] is z_heads[k]) and the
general one (z_tails clones).  Embeddings are N(0,1) * 0.3 and W ~ N(0,1) / sqrt(128), symmetrised: logits of a few units, no
saturated probabilities (the inputs of the other ensemble benches).
  p32          (a) ops.bilinear_ensemble_sigmoid -> fp32
  p16_f16      (b) ... out = a float16 tensor
  p16_bf16     (b) ... out = a bfloat16 tensor
  p32_cast     (c) what was possible before: the fp32 product, then .to(float16) into a second tensor, both resident
Ragged: 4003 x 4003 x 901, K = 2, symmetric and general, into the pitched layout (empty_scores: dword stores of column pairs)
against a contiguous tensor (odd n_tail: rows at 2-byte alignment, every element a 2-byte store), fp32 pitched alongside.
Host destination: N = 4096, 64 outcomes, K = 2, pipeline.ensemble_all_pairs into a numpy array, float32 against float16, wall clock
ending with the last copy.
All variants of a shape run in one process, alternating round by round, after a warm-up call of each; a round times each variant
over a window of at least --window seconds of back-to-back calls with HIP events.  After the timing the float16 tensor is compared
bit for bit with the fp32 product cast, on the first and the last outcome.  ms per call: median [min, max] over the rounds; GB =
bytes of the destination computed from the shape (not from counters), TB/s = GB / ms."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from madrigal_amd import models as M, ops, pipeline  # noqa: E402

PREC = "bf16x3"


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


def run_variants(variants, nbytes, rounds, window_s):
    reps, times = {}, {v: [] for v in variants}
    for v, fn in variants.items():               # warm-up, and the number of calls that fills the window
        fn()
        torch.cuda.synchronize()
        reps[v] = max(1, math.ceil(window_s * 1e3 / max(window_ms(fn, 1), 1e-3)))
    for _ in range(rounds):
        for v, fn in variants.items():
            times[v].append(window_ms(fn, reps[v]))
    res = {}
    for v, ts in times.items():
        ms = float(np.median(ts))
        res[v] = {"ms": round(ms, 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)], "calls_per_window": reps[v],
                  "GB_written": round(nbytes[v] / 1e9, 2), "TBps": round(nbytes[v] / 1e9 / ms, 2)}
    return res


def bench_dense(N, L, Ks, flat32, flat16, rounds, window_s):
    zs, raw = inputs(N, L, max(Ks))
    ws = [ops.symmetrize(w) for w in raw]
    clones = [z.clone() for z in zs]
    out32 = flat32[: L * N * N].view(L, N, N)
    out16 = flat16[: L * N * N].view(L, N, N)
    out16b = out16.view(torch.bfloat16)
    n = L * N * N
    res = {"N": N, "L": L, "precision": PREC, "z_scale": 0.3}
    variants, nbytes = {}, {}
    for K in Ks:
        for sweep, tails in (("sym", zs), ("gen", clones)):
            tag = f"K{K}_{sweep}"

            def cast_route(K=K, tails=tails):
                ops.bilinear_ensemble_sigmoid(zs[:K], tails[:K], ws[:K], precision=PREC, out=out32)
                out16.copy_(out32)
            variants[f"{tag}_p32"] = lambda K=K, tails=tails: ops.bilinear_ensemble_sigmoid(zs[:K], tails[:K], ws[:K], precision=PREC, out=out32)
            variants[f"{tag}_p16_f16"] = lambda K=K, tails=tails: ops.bilinear_ensemble_sigmoid(zs[:K], tails[:K], ws[:K], precision=PREC, out=out16)
            variants[f"{tag}_p16_bf16"] = lambda K=K, tails=tails: ops.bilinear_ensemble_sigmoid(zs[:K], tails[:K], ws[:K], precision=PREC, out=out16b)
            variants[f"{tag}_p32_cast"] = cast_route
            nbytes.update({f"{tag}_p32": 4 * n, f"{tag}_p16_f16": 2 * n, f"{tag}_p16_bf16": 2 * n, f"{tag}_p32_cast": 2 * n})
    res.update(run_variants(variants, nbytes, rounds, window_s))
    ms = lambda nm: res[nm]["ms"]      # noqa: E731
    for K in Ks:
        for sweep in ("sym", "gen"):
            tag = f"K{K}_{sweep}"
            res[f"{tag}_f16_over_p32"] = round(ms(f"{tag}_p16_f16") / ms(f"{tag}_p32"), 4)
            res[f"{tag}_bf16_over_p32"] = round(ms(f"{tag}_p16_bf16") / ms(f"{tag}_p32"), 4)
            res[f"{tag}_f16_over_p32_cast"] = round(ms(f"{tag}_p16_f16") / ms(f"{tag}_p32_cast"), 4)
            # the full-size tensors against each other (offsets past 2^32 bytes): first and last outcome, bit for bit
            variants[f"{tag}_p32"]()
            variants[f"{tag}_p16_f16"]()
            res[f"{tag}_bit_equal_to_p32_cast"] = all(torch.equal(out16[l].view(torch.int16), out32[l].to(torch.float16).view(torch.int16))
                                                      for l in (0, L - 1))
    return res


def bench_ragged(flat32, flat16, rounds, window_s, N=4003, L=901, K=2):
    zs, raw = inputs(N, L, K)
    ws = [ops.symmetrize(w) for w in raw]
    clones = [z.clone() for z in zs]
    pitch = (N + 63) // 64 * 64
    pitched = flat16[: L * N * pitch].view(L, N, pitch)[:, :, :N]
    contig = flat16[: L * N * N].view(L, N, N)
    pitch32 = (N + 31) // 32 * 32
    p32 = flat32[: L * N * pitch32].view(L, N, pitch32)[:, :, :N]
    variants, nbytes = {}, {}
    for sweep, tails in (("sym", zs), ("gen", clones)):
        variants[f"{sweep}_p32_pitched"] = lambda tails=tails: ops.bilinear_ensemble_sigmoid(zs, tails, ws, precision=PREC, out=p32)
        variants[f"{sweep}_f16_pitched"] = lambda tails=tails: ops.bilinear_ensemble_sigmoid(zs, tails, ws, precision=PREC, out=pitched)
        variants[f"{sweep}_f16_contiguous"] = lambda tails=tails: ops.bilinear_ensemble_sigmoid(zs, tails, ws, precision=PREC, out=contig)
        nbytes.update({f"{sweep}_p32_pitched": 4 * L * N * N, f"{sweep}_f16_pitched": 2 * L * N * N, f"{sweep}_f16_contiguous": 2 * L * N * N})
    res = run_variants(variants, nbytes, rounds, window_s)
    res.update({"N": N, "L": L, "K": K, "precision": PREC})
    return res


def bench_host(rounds, N=4096, L=64, K=2):
    zs, raw = inputs(N, L, K)
    dest = {"float32": np.empty((L, N, N), np.float32), "float16": np.empty((L, N, N), np.float16)}
    times = {k: [] for k in dest}
    with M.precision(PREC):
        for rnd in range(rounds + 1):               # round 0 warms up (pinned buffers, page faults of the destination)
            for k, arr in dest.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pipeline.ensemble_all_pairs(raw, zs, out=arr, host_chunk=16)
                dt = (time.perf_counter() - t0) * 1e3
                if rnd:
                    times[k].append(dt)
    return {"N": N, "L": L, "K": K, "precision": PREC, "host_chunk": 16,
            **{k: {"ms": round(float(np.median(ts)), 1), "ms_min_max": [round(min(ts), 1), round(max(ts), 1)],
                   "GB_copied": round(dest[k].nbytes / 1e9, 2)} for k, ts in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--Ks", default="1,2,5")
    ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--L", type=int, default=896)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ensemble_store16_bench needs a GPU"
    N, L = a.N, a.L
    Ks = tuple(int(k) for k in a.Ks.split(","))
    res = {"metric": "bilinear_ensemble_sigmoid16_ms", "unit": "ms", "higher_is_better": False, "device": torch.cuda.get_device_name(0)}
    flat32 = torch.empty(max(L * N * N, 901 * 4003 * 4032), dtype=torch.float32, device="cuda")
    flat16 = torch.empty(max(L * N * N, 901 * 4003 * 4032), dtype=torch.float16, device="cuda")
    res["dense"] = bench_dense(N, L, Ks, flat32, flat16, a.rounds, a.window)
    print("# dense: " + json.dumps(res["dense"]), file=sys.stderr, flush=True)
    res["ragged"] = bench_ragged(flat32, flat16, a.rounds, a.window)
    print("# ragged: " + json.dumps(res["ragged"]), file=sys.stderr, flush=True)
    del flat32, flat16
    torch.cuda.empty_cache()
    if not a.skip_host:
        res["host"] = bench_host(min(a.rounds, 3))
        print("# host: " + json.dumps(res["host"]), file=sys.stderr, flush=True)
    res["value"] = res["dense"][f"K{Ks[-1]}_sym_p16_f16"]["ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
