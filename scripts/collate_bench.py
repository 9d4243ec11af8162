"""Batch collation timing: a synthetic 20 000-drug store, batches of 2048 random drug ids (madrigal/data/data.py:1479-1501 is
what the reference runs on the host for each of them).

(a) ``collate.DeviceCollator`` on its own (ids already on the device, and ids handed over as a host tensor);
(b) the host route it replaces: a vectorised torch gather on CPU tensors, the host-to-device copies, ``molecule_plan`` on the device;
(c) ``PretrainStep.step`` with one fixed batch, with a fresh device-collated batch per step, with a fresh host-collated batch per step.
(d) ``evaluate_pretrain_subsets`` at its 1000-drug cap (str v cv) with either collator.

Medians over the timed calls; every call is timed to a device synchronisation.  Writes profiles/collate_bench.json."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from madrigal_amd import configs, data as D, masks as MK, models as M
from madrigal_amd.collate import DeviceCollator, DrugStore
from madrigal_amd.graph_plans import molecule_plan
from madrigal_amd.optim import AdamW
from madrigal_amd.simclr import SimCLR_NovelDDI
from madrigal_amd.train import PretrainStep

ap = argparse.ArgumentParser()
ap.add_argument("--drugs", type=int, default=20_000)
ap.add_argument("--batch", type=int, default=2048)
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--host-calls", type=int, default=7)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--kg-nodes", type=int, default=130_000)
ap.add_argument("--kg-edges", type=int, default=8_000_000)
ap.add_argument("--precision", default="bf16x3")
ap.add_argument("--skip-steps", action="store_true", help="collation only: no model, no PretrainStep")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "collate_bench.json"))
a = ap.parse_args()


def say(*x):
    print(*x, file=sys.stderr, flush=True)


def timed(fn, n, warm=2):
    """Wall milliseconds of n calls, each up to a device synchronisation."""
    out = []
    for i in range(warm + n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warm:
            out.append((time.perf_counter() - t0) * 1e3)
    return {"ms": round(statistics.median(out), 4), "ms_min_max": [round(min(out), 4), round(max(out), 4)], "calls": n}


M.set_precision(a.precision)
N, B = a.drugs, a.batch
avail = D.make_masks(N, 0)
avail[:, 1] = torch.where(avail[:, 1:].all(dim=1), torch.zeros(N, dtype=torch.bool), avail[:, 1])       # every drug owns a second modality
t0 = time.perf_counter()
batch, bkg = D.make_batch(N, 0, kg_nodes=a.kg_nodes, kg_edges=a.kg_edges, masks=avail)
say(f"synthetic batch of {N} drugs: {time.perf_counter() - t0:.1f} s")
kgc = {"data": bkg["data"].to("cuda"), "drug_index_map": bkg["drug_index_map"].cuda()}
t0 = time.perf_counter()
store = DrugStore.from_batch(D.batch_to(batch, "cuda"), kgc)
torch.cuda.synchronize()
store_build_ms = (time.perf_counter() - t0) * 1e3
collate = DeviceCollator(store)
host = DrugStore.from_batch(batch, bkg)                     # the same arrays on the host, for the host route
rng = np.random.default_rng(0)


def draw_ids():
    return torch.from_numpy(rng.integers(0, N, size=B))


def host_gather(ids):
    """all_molecules[ids], cv[ids], 16 x tx[...][ids] as vectorised torch gathers on CPU tensors."""
    rows = host.id2row[ids]
    B = int(ids.numel())
    na, ne = host.atom_ptr[rows + 1] - host.atom_ptr[rows], host.edge_ptr[rows + 1] - host.edge_ptr[rows]
    oa, oe = torch.zeros(B + 1, dtype=torch.int64), torch.zeros(B + 1, dtype=torch.int64)
    torch.cumsum(na, 0, out=oa[1:])
    torch.cumsum(ne, 0, out=oe[1:])
    g = torch.arange(B)
    n2g, e2g = torch.repeat_interleave(g, na), torch.repeat_interleave(g, ne)
    atoms = torch.arange(int(oa[-1])) + (host.atom_ptr[rows] - oa[:-1])[n2g]
    edges = torch.arange(int(oe[-1])) + (host.edge_ptr[rows] - oe[:-1])[e2g]
    el = host.edge_list[edges]
    el[:, :2] += (oa[:-1] - host.atom_ptr[rows])[e2g][:, None]
    mols = D.MoleculeBatch(host.node_feature[atoms], el, host.edge_feature[edges], n2g, B, host.edge_weight[edges])
    tx = {c: {"sigs": host.sigs[k][rows], "drugs": ids, "dosages": host.dosages[k][rows], "cell_lines": np.full(B, c)} for k, c in enumerate(D.CELL_LINES)}
    return mols, host.cv[rows], tx


def host_route(ids, parts=None):
    t = [time.perf_counter()]
    mols, cv, tx = host_gather(ids)
    t.append(time.perf_counter())
    mols, cv, tx = mols.to("cuda"), cv.cuda(), D.batch_to(tx, "cuda")
    torch.cuda.synchronize()
    t.append(time.perf_counter())
    molecule_plan(mols)
    torch.cuda.synchronize()
    t.append(time.perf_counter())
    if parts is not None:
        parts.append([(y - x) * 1e3 for x, y in zip(t[:-1], t[1:])])
    return ids.cuda(), (mols, kgc, cv, tx)


res = {"metric": "host_route_over_device_collator", "unit": "ratio", "higher_is_better": True, "store_drugs": N, "batch": B,
       "store_atoms": int(store.node_feature.shape[0]), "store_edges": int(store.edge_list.shape[0]), "store_build_ms": round(store_build_ms, 1),
       "launches_per_call": 4, "device_to_host_reads_per_call": 1}

# the two routes agree (edges of the host route are already in the store's order)
ids = draw_ids()
_, (dm, _, dcv, dtx) = collate([ids])
_, (hm, _, hcv, htx) = host_route(ids)
assert torch.equal(dm.node_feature, hm.node_feature) and torch.equal(dm.edge_list, hm.edge_list) and torch.equal(dcv, hcv)
assert all(torch.equal(dtx[c]["sigs"], htx[c]["sigs"]) and torch.equal(dtx[c]["dosages"], htx[c]["dosages"]) for c in D.CELL_LINES)
hp = molecule_plan(hm)
assert all(torch.equal(dm._mdg_plan[k], hp[k]) for k in ("rowptr", "col", "edge_feat_aug", "graph_rowptr"))
out_bytes = sum(t.numel() * t.element_size() for t in (dm.node_feature, dm.edge_list, dm.edge_feature, dm.node2graph, dm.edge_weight, dcv,
                                                      dm._mdg_plan["rowptr"], dm._mdg_plan["col"], dm._mdg_plan["edge_feat_aug"],
                                                      dm._mdg_plan["graph_rowptr"])) + 16 * B * (D.TX_DIM + 1) * 4
res.update(batch_atoms=dm.num_node, batch_edges=dm.num_edge, bytes_written=out_bytes, bytes_moved_estimate=2 * out_bytes)

# (a)
ids_dev = [draw_ids().cuda() for _ in range(a.calls + 2)]
it = iter(ids_dev)
res["device_collator_ids_on_device"] = timed(lambda: collate([next(it)]), a.calls)
ids_host = [draw_ids() for _ in range(a.calls + 2)]
it2 = iter(ids_host)
res["device_collator_ids_on_host"] = timed(lambda: collate([next(it2)]), a.calls)
say("device collator:", res["device_collator_ids_on_device"], res["device_collator_ids_on_host"])
# (b)
parts = []
it3 = iter([draw_ids() for _ in range(a.host_calls + 2)])
res["host_route"] = timed(lambda: host_route(next(it3), parts), a.host_calls)
parts = np.median(np.array(parts[2:]), axis=0)
res["host_route_parts_ms"] = {"cpu_gather": round(float(parts[0]), 3), "host_to_device": round(float(parts[1]), 3), "molecule_plan_on_device": round(float(parts[2]), 3)}
res["value"] = round(res["host_route"]["ms"] / res["device_collator_ids_on_device"]["ms"], 2)
say("host route:", res["host_route"], res["host_route_parts_ms"])

# (c)
if not a.skip_steps:
    torch.manual_seed(0)
    np.random.seed(0)
    enc = configs.build_model("twosides321", bkg["data"], 8).encoder
    model = SimCLR_NovelDDI(enc, dim=128, mlp_dim=512, T=0.1, raw_encoder_output=True).cuda().train()
    bank = MK.get_pretrain_masks(list(range(N)), avail.numpy().astype(np.int64), "str_center_uni", False, 0.2)
    draw = MK.StrCenterUniSampler(bank)
    step = PretrainStep(model, AdamW(model.parameters(), lr=1e-5, weight_decay=1e-2))
    fixed_ids = draw_ids()
    fixed = collate([fixed_ids])

    def run(kind):
        losses = []
        for i in range(a.warmup + a.steps):
            if i == a.warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            if kind in ("fixed", "discard"):
                ids_h, (ids_d, data) = fixed_ids, fixed
                if kind == "discard":               # the collation's own cost inside the loop (its launches and its wait for the device),
                    collate([draw_ids()])           # without the per-batch work a NEW batch causes in the encoder (caches keyed on tensor identity)
            else:
                ids_h = draw_ids()
                ids_d, data = collate([ids_h]) if kind == "device" else host_route(ids_h)
            m1, m2 = draw(ids_h.tolist())
            losses.append(step.step(ids_d, m1, m2, None, data))
        torch.cuda.synchronize()
        return {"ms_per_step": round((time.perf_counter() - t0) / a.steps * 1e3, 3), "steps": a.steps, "last_loss": float(losses[-1])}

    res["pretrain_step"] = {"precision": a.precision, "kg_nodes": a.kg_nodes, "kg_edges": a.kg_edges}
    for kind in ("fixed", "device", "host", "discard", "fixed"):
        key = {"fixed": "fixed_batch", "device": "fresh_device_collated", "host": "fresh_host_collated",
               "discard": "fixed_batch_plus_a_discarded_device_collation"}[kind]
        r = run(kind)
        if key in res["pretrain_step"]:
            key += "_again"
        res["pretrain_step"][key] = r
        say(key, r)

    # (d) evaluate_pretrain_subsets at the 1000-drug cap (str v cv), eval mode: the collator is one part of the call
    from madrigal_amd import evaluate as E
    model.eval()
    all_drugs, all_masks = np.arange(N), avail.numpy().astype(np.int64)
    res["evaluate_pretrain_subsets_1000"] = {}
    for key, col in (("device_collator", collate), ("host_route", lambda arg: host_route(torch.as_tensor(arg[0])))):
        def call(col=col):
            np.random.seed(5)
            E.evaluate_pretrain_subsets(model, all_drugs, all_masks, None, col, [0], [2], "cuda", max_drugs=1000)
        res["evaluate_pretrain_subsets_1000"][key] = timed(call, 7)
        say("evaluate_pretrain_subsets", key, res["evaluate_pretrain_subsets_1000"][key])

os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write(json.dumps(res) + "\n")
print(json.dumps(res))
