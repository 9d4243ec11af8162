"""The KG encoder's convs at the bench shape (130 000 nodes, 8e6 edges, 2 HGT convs, only the drug rows of the last one
read), inference, alone on the device: each conv as a whole and, inside it, its edge-attention launch (HGTConv's
``_attention_probe`` events), so that the two ``hgt_attention_kernel`` launches of a step -- the first conv over every destination
type, the last conv over the drug destinations only -- are known apart and the last conv splits into projection + output
blocks | attention.  Device events, median of --reps forwards; the plan of each conv also gives its edge and destination counts.
Measured twice: with the k' | v' rows of every node projected (``attend_in_feature_space`` off) and with the last conv attending
in node-feature space (its "attention" is then the feature-space kernel and its combine; the two dense blocks beside it count
as the rest), and the drug rows of the two are compared.

    python scripts/kg_last_conv_bench.py [--out profiles/featspace_last_conv.json] [--nodes 130000] [--edges 8000000] [--reps 20]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madrigal_amd import configs, data as D, models as M      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/featspace_last_conv.json")
    ap.add_argument("--drugs", type=int, default=4096)
    ap.add_argument("--nodes", type=int, default=130_000)
    ap.add_argument("--edges", type=int, default=8_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--precision", default="bf16x3")
    a = ap.parse_args()
    _, bkg = D.make_batch(a.drugs, 0, kg_nodes=a.nodes, kg_edges=a.edges)
    torch.manual_seed(1234)
    enc = configs.build_model("twosides321", bkg["data"], 8).encoder.kg_encoder.cuda().eval()
    kg = bkg["data"].to("cuda")
    convs = list(enc.convs)
    ev = lambda: torch.cuda.Event(enable_timing=True)            # noqa: E731
    probes = [{"start": ev(), "end": ev()} for _ in convs]
    marks = [(ev(), ev()) for _ in convs]
    whole = (ev(), ev())

    def forward():
        last = len(convs) - 1
        whole[0].record()
        out = kg.x_dict
        for i, conv in enumerate(convs):                         # HGT.forward, with events between the convs
            marks[i][0].record()
            out = conv(out, kg.edge_index_dict, needed_types=("drug",) if i == last else None)
            if 0 < i < last:
                out = {t: torch.relu_(x) for t, x in out.items()}
            marks[i][1].record()
        whole[1].record()
        return out["drug"]

    def measure(feature_space: bool) -> dict:
        times = {f"conv{i}": [] for i in range(len(convs))}
        times.update({f"conv{i}_attention": [] for i in range(len(convs))})
        times["both_convs"] = []
        with torch.no_grad(), M.precision(a.precision):
            for i, conv in enumerate(convs):
                conv.__dict__["_attention_probe"] = probes[i]
                conv.attend_in_feature_space = feature_space
            for rep in range(a.reps + 3):
                rows = forward()
                torch.cuda.synchronize()
                if rep < 3:
                    continue
                for i in range(len(convs)):
                    times[f"conv{i}"].append(marks[i][0].elapsed_time(marks[i][1]))
                    times[f"conv{i}_attention"].append(probes[i]["start"].elapsed_time(probes[i]["end"]))
                times["both_convs"].append(whole[0].elapsed_time(whole[1]))
            for conv in convs:
                conv.__dict__.pop("_attention_probe", None)
        res = {"ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()},
               "attention_launch": {f"conv{i}": {"edges": p["edges"], "destination_rows": p["dst_rows"], "buffer_MB": p["buffer_floats"] * 4 / 1e6}
                                    for i, p in enumerate(probes)}}
        for i in range(len(convs)):
            res["ms"][f"conv{i}_everything_but_attention"] = {"median": res["ms"][f"conv{i}"]["median"] - res["ms"][f"conv{i}_attention"]["median"]}
        return res, rows.clone()

    # the last conv with its k' | v' rows projected for every node (attend_in_feature_space off), then attending in feature space
    projected, rows_p = measure(False)
    feature, rows_f = measure(True)
    res = {"device": torch.cuda.get_device_name(0), "precision": a.precision, "nodes": a.nodes, "reps": a.reps, "drug_rows": int(rows_p.shape[0]),
           "projected": projected, "feature_space": feature,
           "max_abs_difference_over_scale": float((rows_f - rows_p).abs().max() / rows_p.abs().max())}
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
