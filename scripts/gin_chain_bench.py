"""The GIN structure encoder alone at the bench shape (4096 drugs, ~106k atoms, 4 layers x 3-layer MLP, width 128), inference:
one dense block per launch (fuse_layer_chain = False) against one mdg_linear_chain128 launch per layer (True), in bf16x3 and
bf16.  Device events, median of 20 forwards; the outputs of the two paths are compared bit for bit.

    python scripts/gin_chain_bench.py [--out profiles/ginchain_bench.json] [--drugs 4096] [--reps 20]

MDG_CHAIN_ROWS=128 selects the 128-row panel (default 64); the script times both."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madrigal_amd import _lib, configs, data as D, models as M      # noqa: E402


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/ginchain_bench.json")
    ap.add_argument("--drugs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    mols = D.make_molecules(a.drugs, seed=0).cuda()
    hp = configs.GIN
    torch.manual_seed(0)
    gin = M.GraphIsomorphismNetwork(input_dim=67, hidden_dims=hp["gin_hidden_dims"] + [128], edge_input_dim=hp["gin_edge_input_dim"],
                                    num_mlp_layer=hp["gin_num_mlp_layer"], eps=hp["gin_eps"], batch_norm=hp["gin_batch_norm"],
                                    activation=hp["gin_actn"], readout=hp["gin_readout"]).cuda().eval()
    x = mols.node_feature.float()
    res = {"atoms": int(x.shape[0]), "drugs": a.drugs, "reps": a.reps, "device": torch.cuda.get_device_name(0), "modes": {}}

    def fwd():
        return gin(mols, x)
    with torch.no_grad():
        for prec in ("bf16x3", "bf16"):
            with M.precision(prec):
                row = {}
                gin.fuse_layer_chain = False
                want = fwd()["node_feature"].clone()
                row["unfused"] = timed(fwd, a.reps)
                gin.fuse_layer_chain = True
                for rows in ("64", "128"):
                    os.environ["MDG_CHAIN_ROWS"] = rows
                    _lib.lib().mdg_tuning_reload()
                    same = bool(torch.equal(fwd()["node_feature"], want))
                    row[f"fused_panel{rows}"] = dict(timed(fwd, a.reps), bit_equal=same)
                os.environ.pop("MDG_CHAIN_ROWS")
                _lib.lib().mdg_tuning_reload()
                row["fused_default"] = dict(timed(fwd, a.reps), bit_equal=bool(torch.equal(fwd()["node_feature"], want)))
                res["modes"][prec] = row
                print(prec, json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
