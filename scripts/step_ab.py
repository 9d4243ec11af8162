#!/usr/bin/env python3
"""The headline step of a parent checkout against this tree, alternating in one call (run on the GPU box):

    python3 scripts/step_ab.py --parent DIR [--runs 3] [--out profile_out/step_ab.json]

DIR holds the parent commit's tree with its own built library.  Each run is `bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs D`
in a process of its own, un-profiled, parent first; the JSON (the format of profiles/*_step_ab.json) lists ms_per_step,
encode_fuse_ms and the head's kernel_ms of every run, and max|d| / max|.| of the change's embeddings.npy and scores_sample.npy
against the parent's (last run of each).  A run that fails ends the script: nothing is started after it.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(tree: str, dump: str, timeout: int) -> dict:
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3", "--dump-outputs", dump]
    r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"bench.py in {tree} ended with status {r.returncode}")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"ms_per_step"' in ln]
    return json.loads(lines[-1])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per bench.py run")
    ap.add_argument("--out", default="profile_out/step_ab.json")
    args = ap.parse_args()
    trees = {"parent": os.path.abspath(args.parent), "change": HERE}
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(1, args.runs + 1):
            for build, tree in trees.items():
                line = bench(tree, os.path.join(tmp, build), args.timeout)
                runs.append({"build": build, "run": i, "ms_per_step": line["ms_per_step"], "encode_fuse_ms": line["roofline"]["encode_fuse_ms"],
                             "head_kernel_ms": line["roofline"]["kernel_ms"]})
                print(json.dumps(runs[-1]), flush=True)
        outputs = {}
        for name in ("embeddings.npy", "scores_sample.npy"):
            a, b = (np.load(os.path.join(tmp, build, name)).astype(np.float64) for build in ("parent", "change"))
            outputs[name] = {"max_abs_diff_over_max_abs": float(np.abs(a - b).max() / np.abs(a).max()), "bit_equal": bool(np.array_equal(a, b))}
    res = {"command": f"bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs DIR, parent and change alternating in one call, {args.runs} runs "
                      "each (un-profiled)", "runs": runs, "outputs_change_against_parent": outputs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(outputs))


if __name__ == "__main__":
    main()
