#!/usr/bin/env python3
"""Record tests/golden/lars_reference.npz from the REFERENCE's own LARS (madrigal/utils.py:628-662).

TEST INFRASTRUCTURE ONLY: needs a checkout of the reference; no GPU.
    python scripts/gen_optim_golden.py --ref <reference checkout> [--out tests/golden/lars_reference.npz]

The reference is imported through oracle.gen_golden.import_reference (third-party layers shimmed); its ``madrigal.utils.LARS`` runs
the input set of tests/lars_ref.py for 6 steps on the CPU, once in fp32 (recorded) and once on float64 copies of the same inputs.
The fixture holds recorded numbers only: the seeds, the final parameters and every ``mu`` of the fp32 run (the two large tensors as
every STRIDE-th element, tests/lars_ref.py), the key sets of the optimizer's ``state_dict`` and the worst distance between the fp32
and the float64 run under the measure the tests use, over exactly the recorded entries -- how far the reference's own fp32
arithmetic (its ``torch.norm``) is from exact.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lars_ref as R  # noqa: E402
from oracle.gen_golden import import_reference  # noqa: E402


def run(LARS, dtype):
    ps = [torch.nn.Parameter(p) for p in R.initial_params(dtype)]
    opt = LARS(R.param_groups(ps), **R.DEFAULTS)
    for s in range(R.STEPS):
        for i, p in enumerate(ps):
            p.grad = R.grad(s, i, dtype)
        opt.step()
    return ps, opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lars_reference.npz"))
    args = ap.parse_args()
    import_reference(args.ref)
    from madrigal.utils import LARS
    p32, opt32 = run(LARS, torch.float32)
    p64, opt64 = run(LARS, torch.float64)
    out = {"steps": np.int64(R.STEPS), "param_seed": np.int64(R.PARAM_SEED),
           "grad_seeds": np.asarray([[100 * s + i for i in range(len(p32))] for s in range(R.STEPS)], dtype=np.int64),
           "stride": np.asarray([R.STRIDE.get(i, 1) for i in range(len(p32))], dtype=np.int64)}
    worst = {"p": 0.0, "mu": 0.0}
    for i, (a, b) in enumerate(zip(p32, p64)):
        for name, x32, x64 in (("p", a.detach(), b.detach()), ("mu", opt32.state[a]["mu"], opt64.state[b]["mu"])):
            x32, x64 = R.stored(i, x32), R.stored(i, x64)
            out[f"{name}_{i}"] = x32.numpy().copy()
            d = R.distance(x64, x32)
            worst[name] = max(worst[name], d)
            print(f"tensor {i:2d} {str(R.SHAPES[i]):16s} {name:2s} fp32 vs float64: {d:.3e}")
    sd = opt32.state_dict()
    out["state_keys"] = np.asarray(sorted({k for st in sd["state"].values() for k in st}))
    out["group_keys"] = np.asarray(sorted(k for k in sd["param_groups"][0] if k != "params"))
    out["n_state"] = np.int64(len(sd["state"]))
    out["worst_p"], out["worst_mu"] = np.float64(worst["p"]), np.float64(worst["mu"])
    np.savez_compressed(args.out, **out)
    print(f"worst p {worst['p']:.3e}, worst mu {worst['mu']:.3e}; {args.out}: {os.path.getsize(args.out) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
