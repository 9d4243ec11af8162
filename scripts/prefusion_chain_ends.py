"""Where the two chains of the inference step's pre-fusion window end, from a rocprofv3 --kernel-trace CSV of bench.py's
headline loop: per step (one step = up to and including an all-pairs head launch) the time from the step's first kernel to
- the end of the KG queue's last kernel (the queue the HGT attention runs on), and
- the end of the last kernel that the main queue (the head's queue) started before that moment.
The main queue waits for the KG rows there, so its later kernels belong to the fusion.  Median over the last --steps steps.

    python scripts/prefusion_chain_ends.py <kernel_trace.csv> [--steps 12] [--out chains.json]"""
import argparse
import csv
import json
import statistics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"], r["Kernel_Name"]) for r in csv.DictReader(open(a.trace))]
    rows.sort()
    heads = [i for i, r in enumerate(rows) if "bilinear_allpairs" in r[3]]
    kg_q = {r[2] for r in rows if "hgt_attention" in r[3]}
    main_q = {rows[i][2] for i in heads}
    per_step = []
    for prev, cur in zip(heads[:-1], heads[1:]):
        step = rows[prev + 1: cur]
        kg = [r for r in step if r[2] in kg_q and r[2] not in main_q]
        if not step or not kg:
            continue
        t0 = step[0][0]
        kg_end = max(r[1] for r in kg)
        main_before = [r for r in step if r[2] in main_q and r[0] < kg_end]
        last_kg = max(kg, key=lambda r: r[1])[3]
        per_step.append({"kg_queue_end_us": (kg_end - t0) / 1e3, "main_queue_end_us": (max(r[1] for r in main_before) - t0) / 1e3 if main_before else 0.0,
                         "kg_kernel_us": sum(r[1] - r[0] for r in kg) / 1e3, "kg_launches": len(kg), "last_kg_kernel": last_kg.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0].split("<")[0]})
    per_step = per_step[-a.steps:]
    res = {"steps": len(per_step), "separate_queues": bool(kg_q - main_q)}
    for k in ("kg_queue_end_us", "main_queue_end_us", "kg_kernel_us", "kg_launches"):
        res[k] = statistics.median(s[k] for s in per_step) if per_step else None
    res["last_kg_kernel"] = per_step[-1]["last_kg_kernel"] if per_step else None
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
