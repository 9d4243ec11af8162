"""Checkpoint-ensembled probabilities at the headline size: 4096 drugs x 896 outcomes, K checkpoints, one fused sweep
(ops.bilinear_ensemble_sigmoid) against the composed path measured beside it (per outcome chunk: K single-model launches with the
sigmoid epilogue into a [K, chunk, N, N] buffer, then torch's mean over the models), alternated launch by launch.

    python scripts/ensemble_bench.py [--reps 3] [--quick]      -> one JSON line on stdout

Per entry: device-event ms per ensemble (median of --reps after one warm-up), probabilities/s, the composed baseline, and the roofline
-- the larger of the matrix work over the matrix peak (2.5 PF bf16 for the three bf16 products of bf16x3, 157 TF fp32) and the
4 B per probability of stores over 8 TB/s (MI355X_MICROARCH.md) -- with which of the two bounds it.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from madrigal_amd import ops  # noqa: E402

PEAK = {"bf16x3": 2.5e15, "f32": 157e12}
PRODUCTS = {"bf16x3": 3, "f32": 1}
HBM_STORE = 8e12


def roofline(K, N, L, prec, sym):
    flop = 2.0 * PRODUCTS[prec] * L * N * N * 128 * K * (0.5 if sym else 1.0)
    t_mfma = flop / PEAK[prec]
    t_store = L * N * N * 4 / HBM_STORE
    return {"mfma_ms": round(t_mfma * 1e3, 2), "store_ms": round(t_store * 1e3, 2), "roofline_ms": round(max(t_mfma, t_store) * 1e3, 2),
            "bound": "mfma" if t_mfma >= t_store else "store"}


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--L", type=int, default=896)
    ap.add_argument("--chunk", type=int, default=64, help="outcomes per chunk of the composed baseline")
    ap.add_argument("--quick", action="store_true", help="the fused K = 5 bf16x3 symmetric launch only (for a kernel-trace run)")
    a = ap.parse_args()
    N, L = a.N, a.L
    g = torch.Generator().manual_seed(0)
    zs = [torch.randn(N, 128, generator=g).cuda() for _ in range(5)]
    ws = [ops.symmetrize((torch.randn(L, 128, 128, generator=g) / 128 ** 0.5).cuda()) for _ in range(5)]
    out = ops.empty_scores(L, N, N, "cuda")
    cases = [(1, "bf16x3"), (2, "bf16x3"), (5, "bf16x3"), (5, "f32")]
    if a.quick:
        cases = [(5, "bf16x3")]
    stack = None if a.quick else torch.empty((5, a.chunk, N, N), dtype=torch.float32, device="cuda")
    entries = []
    for K, prec in cases:
        for sym in (True, False):
            if a.quick and not sym:
                continue
            zh = zs[:K]
            zt = zh if sym else [z.clone() for z in zh]
            fused = lambda: ops.bilinear_ensemble_sigmoid(zh, zt, ws[:K], precision=prec, out=out)  # noqa: E731

            def composed():
                for s in range(0, L, a.chunk):
                    e = min(L, s + a.chunk)
                    for k in range(K):
                        ops.bilinear_allpairs(zh[k], zt[k], ws[k][s:e], precision=prec, epilogue=ops.EPI_STORE_SIGMOID, out=stack[k, : e - s])
                    torch.mean(stack[:K, : e - s], dim=0, out=out[s:e])

            fused()
            if a.quick:
                torch.cuda.synchronize()
                timed(fused)
                continue
            composed()
            tf, tc = [], []
            for _ in range(a.reps):                       # alternated: fused, composed, fused, ...
                tf.append(timed(fused))
                tc.append(timed(composed))
            mf, mc = statistics.median(tf), statistics.median(tc)
            ent = {"K": K, "precision": prec, "sweep": "symmetric" if sym else "general", "fused_ms": round(mf, 2),
                   "probs_per_s": float(f"{L * N * N / (mf * 1e-3):.3e}"), "composed_ms": round(mc, 2), "speedup": round(mc / mf, 2),
                   "fused_ms_all": [round(x, 2) for x in tf], "composed_ms_all": [round(x, 2) for x in tc]}
            ent.update(roofline(K, N, L, prec, sym))
            ent["fraction_of_roofline"] = round(ent["roofline_ms"] / mf, 3)
            entries.append(ent)
            print(json.dumps(ent), file=sys.stderr, flush=True)
    if a.quick:
        print(json.dumps({"quick": True}))
        return
    print(json.dumps({"workload": f"ensemble of K checkpoints, {N} drugs x {L} outcomes, [L,N,N] fp32 probabilities in HBM",
                      "device": torch.cuda.get_device_name(0), "reps": a.reps, "entries": entries}))


if __name__ == "__main__":
    main()
