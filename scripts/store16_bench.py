#!/usr/bin/env python3
"""Time the 16-bit destinations of the all-pairs head (csrc/store16.hip, mdg_bilinear_allpairs16_ld) against the fp32 head, against
the only route to a 16-bit tensor that existed before it (fp32 head + cast) and against the bare sweep.  Prints one JSON line
(recorded as profiles/store16_bench.json).

    python scripts/store16_bench.py [--rounds 5] [--modes bf16x3,bf16,f16] [--out FILE]

Per precision mode at 4096 x 4096 drugs x 896 outcomes (BASELINE configs[1]):
  store32          ops.bilinear_allpairs -> fp32, GENERAL sweep (z_tail a clone): the kernel the 16-bit sweep shares its arithmetic with
  store32_sym      the same as users call it (z_head is z_tail): the fp32 launcher's symmetric sweep
  store32_cast     the route that existed before: the fp32 head on blocks of head rows sized to a 16 GB buffer (what
                   pipeline.score_all_pairs(head_rows=...) launches) and .to(float16) of every block into the 16-bit tensor
  store16_f16 / store16_bf16 / sigmoid16_f16    ops.bilinear_allpairs(out=16-bit tensor), EPI_STORE / EPI_STORE_SIGMOID
  rowstats         EPI_ROWSTATS: the bare sweep, nothing materialised (the floor)
Ragged, per mode: 4003 x 4003 x 901 into the pitched layout (empty_scores: dword stores of column pairs) against a contiguous
tensor (odd n_tail: rows at 2-byte alignment, every element a 2-byte store) -- what that path costs.
Host destination (bf16x3): N = 4096, 64 outcomes, pipeline.score_all_pairs into a numpy array, float32 against float16, wall
clock ending with the last copy.
All variants of a shape run in one process, alternating round by round; a round times each variant over a window of at least
--window seconds of back-to-back calls with HIP events.  After the timing the float16 tensor is compared bit for bit with the general
fp32 sweep cast, on the first and the last outcome (`bit_equal_to_store32_cast`).  ms per call: median [min, max] over the rounds; GB = bytes of the
destination computed from the shape (not from counters), TB/s = GB / ms."""
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
        res[v] = {"ms": round(ms, 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)], "calls_per_window": reps[v]}
        if nbytes.get(v):
            res[v]["GB_written"] = round(nbytes[v] / 1e9, 2)
            res[v]["TBps"] = round(nbytes[v] / 1e9 / ms, 2)
    return res


def bench_mode(prec, z, w, flat32, flat16, rounds, window_s):
    N, L = z.shape[0], w.shape[0]
    zc = z.clone()
    out32 = flat32[: L * N * N].view(L, N, N)
    out16 = flat16[: L * N * N].view(L, N, N)
    out16b = out16.view(torch.bfloat16)
    block = max(1, min(N, (16 << 30) // (L * N * 4)))
    cast_buf = torch.empty(L * block * N, dtype=torch.float32, device="cuda")

    def cast_route():
        for r0 in range(0, N, block):
            r1 = min(N, r0 + block)
            s = ops.bilinear_allpairs(z[r0:r1], z, w, precision=prec, out=cast_buf[: L * (r1 - r0) * N].view(L, r1 - r0, N))
            out16[:, r0:r1].copy_(s)

    variants = {
        "store32": lambda: ops.bilinear_allpairs(z, zc, w, precision=prec, out=out32),
        "store32_sym": lambda: ops.bilinear_allpairs(z, z, w, precision=prec, out=out32),
        "store32_cast": cast_route,
        "store16_f16": lambda: ops.bilinear_allpairs(z, z, w, precision=prec, out=out16),
        "store16_bf16": lambda: ops.bilinear_allpairs(z, z, w, precision=prec, out=out16b),
        "sigmoid16_f16": lambda: ops.bilinear_allpairs(z, z, w, precision=prec, epilogue=ops.EPI_STORE_SIGMOID, out=out16),
        "rowstats": lambda: ops.bilinear_allpairs(z, z, w, precision=prec, epilogue=ops.EPI_ROWSTATS),
    }
    n = L * N * N
    nbytes = {"store32": 4 * n, "store32_sym": 4 * n, "store32_cast": 2 * n, "store16_f16": 2 * n, "store16_bf16": 2 * n, "sigmoid16_f16": 2 * n}
    res = run_variants(variants, nbytes, rounds, window_s)
    res["store32_cast_row_block"] = block
    # the full-size tensors against each other (offsets past 2^32 bytes): first and last outcome, bit for bit
    variants["store32"]()
    variants["store16_f16"]()
    res["bit_equal_to_store32_cast"] = all(torch.equal(out16[l].view(torch.int16), out32[l].to(torch.float16).view(torch.int16)) for l in (0, L - 1))
    del cast_buf
    return res


def bench_ragged(prec, flat16, rounds, window_s, N=4003, L=901):
    z = torch.randn(N, 128, generator=torch.Generator().manual_seed(2)).cuda()
    w = ops.symmetrize((torch.randn(L, 128, 128, generator=torch.Generator().manual_seed(3)) / 128 ** 0.5).cuda())
    pitch = (N + 63) // 64 * 64
    pitched = flat16[: L * N * pitch].view(L, N, pitch)[:, :, :N]
    contig = flat16[: L * N * N].view(L, N, N)
    variants = {"pitched": lambda: ops.bilinear_allpairs(z, z, w, precision=prec, out=pitched),
                "contiguous": lambda: ops.bilinear_allpairs(z, z, w, precision=prec, out=contig)}
    n = 2 * L * N * N
    res = run_variants(variants, {"pitched": n, "contiguous": n}, rounds, window_s)
    res.update({"N": N, "L": L})
    return res


def bench_host(rounds, N=4096, L=64):
    model = DecoderOnly(L, 0).cuda().eval()
    z = torch.randn(N, 128, generator=torch.Generator().manual_seed(1)).cuda()
    dest = {"float32": np.empty((L, N, N), np.float32), "float16": np.empty((L, N, N), np.float16)}
    times = {k: [] for k in dest}
    with M.precision("bf16x3"):
        for rnd in range(rounds + 1):               # round 0 warms up (pinned buffers, page faults of the destination)
            for k, arr in dest.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pipeline.score_all_pairs(model, z, out=arr, host_chunk=16)
                dt = (time.perf_counter() - t0) * 1e3
                if rnd:
                    times[k].append(dt)
    return {"N": N, "L": L, "precision": "bf16x3", "host_chunk": 16,
            **{k: {"ms": round(float(np.median(ts)), 1), "ms_min_max": [round(min(ts), 1), round(max(ts), 1)],
                   "GB_copied": round(dest[k].nbytes / 1e9, 2)} for k, ts in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--modes", default="bf16x3,bf16,f16")
    ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--L", type=int, default=896)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "store16_bench needs a GPU"
    N, L = a.N, a.L
    res = {"metric": "bilinear_store16_ms", "unit": "ms", "higher_is_better": False, "N": N, "L": L}
    z = torch.randn(N, 128, generator=torch.Generator().manual_seed(1)).cuda()
    w = ops.symmetrize((torch.randn(L, 128, 128, generator=torch.Generator().manual_seed(0)) / 128 ** 0.5).cuda())
    flat32 = torch.empty(L * N * N, dtype=torch.float32, device="cuda")
    flat16 = torch.empty(max(L * N * N, 901 * 4003 * 4032), dtype=torch.float16, device="cuda")
    for prec in a.modes.split(","):
        res[prec] = bench_mode(prec, z, w, flat32, flat16, a.rounds, a.window)
        print(f"# {prec}: " + json.dumps(res[prec]), file=sys.stderr, flush=True)
    res["ragged"] = {}
    for prec in a.modes.split(","):
        res["ragged"][prec] = bench_ragged(prec, flat16, a.rounds, a.window)
        print(f"# ragged {prec}: " + json.dumps(res["ragged"][prec]), file=sys.stderr, flush=True)
    del flat32, flat16
    torch.cuda.empty_cache()
    if not a.skip_host:
        res["host"] = bench_host(min(a.rounds, 3))
        print("# host: " + json.dumps(res["host"]), file=sys.stderr, flush=True)
    first = a.modes.split(",")[0]
    res["value"] = res[first]["store16_f16"]["ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
