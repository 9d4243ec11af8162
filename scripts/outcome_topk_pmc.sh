#!/bin/bash
# One SQ counter pass over the outcome top-k kernel at the bench shape (run on the GPU box; counters in a run of their own, no tracing):
#   bash scripts/outcome_topk_pmc.sh <outdir> [dtype=bfloat16] [k=5]
# Writes <outdir>/summary.json: per counter the mean over the kernel's dispatches, and the shares of the wave cycles.
set -e
out=$1; dtype=${2:-bfloat16}; k=${3:-5}
export TMPDIR=/tmp
mkdir -p $out
timeout -k 10 400 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAVES \
  --output-format csv -d $out/pmc -- python3 scripts/outcome_topk_bench.py --parts kernel --dtypes $dtype --k $k > $out/pmc.log 2>&1
python3 - "$out" "$dtype" "$k" <<'PY'
import collections, csv, glob, json, sys
out, dtype, k = sys.argv[1], sys.argv[2], int(sys.argv[3])
agg = collections.defaultdict(list)
for f in glob.glob(f"{out}/pmc/*/*_counter_collection.csv"):
    for r in csv.DictReader(open(f)):
        if "outcome_topk_kernel" in r["Kernel_Name"]:
            agg[r["Counter_Name"]].append(float(r["Counter_Value"]))
res = {"dtype": dtype, "k": k, "dispatches": {c: len(v) for c, v in agg.items()}, "mean": {c: sum(v) / len(v) for c, v in agg.items()}}
m = res["mean"]
if m.get("SQ_WAVE_CYCLES"):
    res["share_of_wave_cycles"] = {c: round(m[c] / m["SQ_WAVE_CYCLES"], 4) for c in ("SQ_ACTIVE_INST_ANY", "SQ_ACTIVE_INST_VALU", "SQ_WAIT_ANY",
                                                                                   "SQ_WAIT_INST_ANY") if c in m}
json.dump(res, open(f"{out}/summary.json", "w"))
print(json.dumps(res))
PY
