"""Where the pre-fusion phase of the inference step goes, per stream, at the bench shape (device events, median of N):
the main stream's chain (structure GIN, cv MLP, tx encoder) and the KG stream's chain (HGT), each alone, then the whole
encoder with ``overlap_kg`` on and off -- with the GIN layer chain fused and unfused.

    python scripts/encode_chain_times.py [--out profiles/ginchain_phase_times.json] [--reps 20]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madrigal_amd import configs, data as D, models as M      # noqa: E402


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
    return round(statistics.median(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/ginchain_phase_times.json")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    N, L = 4096, 896
    batch, bkg = D.make_batch(N, 0, kg_nodes=130000, kg_edges=8000000)
    model = configs.build_model("twosides321", bkg["data"], L).cuda().eval()
    b = D.batch_to(batch, "cuda")
    kgc = {"data": bkg["data"].to("cuda"), "drug_index_map": bkg["drug_index_map"].cuda()}
    enc = model.encoder
    filler = torch.randn(N, 128, device="cuda")
    x = b["strs"].node_feature.float()
    res = {"reps": a.reps, "atoms": int(x.shape[0]), "ms": {}}
    with torch.no_grad(), M.precision("bf16x3"):
        for fuse in (False, True):
            enc.str_encoder.fuse_layer_chain = fuse
            r = {"gin": timed(lambda: enc.str_encoder(b["strs"], x), a.reps),
                 "cv": timed(lambda: enc.cv_encoder(b["cv"]), a.reps),
                 "tx": timed(lambda: enc._encode_tx(b["tx"], N, "cuda"), a.reps),
                 "kg": timed(lambda: enc.kg_encoder(kgc["data"].x_dict, kgc["data"].edge_index_dict), a.reps)}
            r["main_chain"] = round(r["gin"] + r["cv"] + r["tx"], 4)
            for ov in (True, False):
                enc.overlap_kg = ov
                r[f"encoder_overlap_{ov}"] = timed(lambda: enc(b["drugs"], b["masks"], b["strs"], kgc, b["cv"], b["tx"], kg_filler=filler), a.reps)
            enc.overlap_kg = True
            res["ms"]["fused" if fuse else "unfused"] = r
            print("fused" if fuse else "unfused", json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
