#!/usr/bin/env python3
"""The two small kernels in the fusion transformer's tail, each alone, at the flagship shape (run on the GPU box):

    python3 scripts/fusion_tail_bench.py                       # this tree: one JSON line
    python3 scripts/fusion_tail_bench.py --against DIR [--out profile_out/fusion_tail_bench.json]

  layernorm_logits    x_attn_kv_norm with the H key logits: 8 192 kept rows, d = 2048, H = 8, bf16x3 image
  token_scaled_rows   layer 0's token rows: 22 016 live rows, D = 128, R_f [129, 132]

Device events around one launch, median of 20 after 5 warm-up launches.  --against: DIR holds another checkout with its own built
library; the two trees alternate, three processes each, and the JSON lists every process's medians.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(tree: str) -> dict:
    sys.path.insert(0, tree)
    import torch
    from madrigal_amd import ops
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(8192, 2048, generator=g) * 2 + 0.5).cuda()
    w, b = (1 + 0.1 * torch.randn(2048, generator=g)).cuda(), (0.1 * torch.randn(2048, generator=g)).cuda()
    G = (torch.randn(8, 2048, generator=g) / 45).cuda()
    tok = torch.randn(22016, 128, generator=g).cuda()
    rf = torch.triu(torch.randn(129, 132, generator=g)).cuda().contiguous()
    tail = torch.empty(22016, 128, device="cuda")
    cases = {"layernorm_logits_us": lambda: ops.layernorm_logits(x, w, b, 1e-5, G, "bf16x3"),
             "token_scaled_rows_us": lambda: ops.token_scaled_rows(tok, rf, 2048, 1e-5, tail)}
    out = {}
    with torch.no_grad():
        for name, fn in cases.items():
            for _ in range(5):
                fn()
            ts = []
            for _ in range(20):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            out[name] = sorted(ts)[len(ts) // 2]
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--against")
    ap.add_argument("--out", default="profile_out/fusion_tail_bench.json")
    args = ap.parse_args()
    if not args.against:
        print(json.dumps(measure(os.path.abspath(args.tree))), flush=True)
        return
    runs = []
    for i in range(1, 4):
        for build, tree in (("parent", os.path.abspath(args.against)), ("change", HERE)):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree], capture_output=True, text=True, timeout=240)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"{build}: ended with status {r.returncode}")
            runs.append({"build": build, "run": i, **json.loads(r.stdout.strip().splitlines()[-1])})
            print(json.dumps(runs[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"what": "device events around one launch, median of 20, microseconds; parent and change alternating, one process each",
                   "runs": runs}, f, indent=1)


if __name__ == "__main__":
    main()
