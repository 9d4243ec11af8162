"""Optimizer-step timing on the GPU: optim.LARS / optim.RAdam / optim.AdamW against what was possible before them.

Two parameter sets with random gradients: the SimCLR model of BASELINE configs[2] (contrastive pretraining) and the TWOSIDES finetune
model (896 outcomes).  Variants, alternated round by round within this one process, each on its own copy of the parameters:
    lars_hip / radam_hip / adamw_hip    one step() of the HIP path (3 / 1 / 1 launches)
    lars_torch_loop                     the LARS algorithm as a per-tensor torch-op loop on the GPU (no host read-back)
    radam_torch_foreach                 torch.optim.RAdam(foreach=True)
Every variant is warmed up, then timed with device events over rounds of back-to-back steps until its windows add up to at least
``--window`` seconds; the figure is the median round.  bytes/s is the 28 B/element count (LARS: 8 B in the norm pass + 20 B in the
update; Adam family: 4 tensors read, 3 written) over that time -- a byte count over a measured time, not a counter reading.
Last, a whole PretrainStep (batch 2048, the configs[2] KG) with LARS against AdamW over the same model, alternated the same way.

    python scripts/optim_bench.py [--out profiles/optim_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from madrigal_amd import configs, data as D, masks as MK, models as M  # noqa: E402
from madrigal_amd.optim import LARS, AdamW, RAdam  # noqa: E402
from madrigal_amd.simclr import SimCLR_NovelDDI  # noqa: E402
from madrigal_amd.train import PretrainStep  # noqa: E402


class TorchLoopLARS:
    """LARS tensor by tensor in torch ops: the trust ratio stays on the device (torch.where), as a user of the reference would run it."""

    def __init__(self, params, lr, weight_decay, momentum, trust_coefficient):
        self.params, self.hp, self.mu = list(params), (lr, weight_decay, momentum, trust_coefficient), {}

    @torch.no_grad()
    def step(self):
        lr, wd, momentum, tc = self.hp
        for p in self.params:
            u = p.grad
            if u is None:
                continue
            if p.ndim > 1:
                u = torch.add(u, p, alpha=wd)
                pn, un = torch.linalg.vector_norm(p), torch.linalg.vector_norm(u)
                u = u * torch.where((pn > 0) & (un > 0), tc * pn / un, torch.ones_like(pn))
            mu = self.mu.get(p)
            if mu is None:
                mu = self.mu[p] = torch.zeros_like(p)
            mu.mul_(momentum).add_(u)
            p.add_(mu, alpha=-lr)


def copies(params):
    out = [torch.nn.Parameter(p.detach().clone()) for p in params]
    for i, p in enumerate(out):
        p.grad = torch.randn(p.shape, device=p.device, generator=torch.Generator(p.device).manual_seed(i)) * 1e-2
    return out


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def alternate(variants, window, round_s=0.1, warmup=5):
    """variants: name -> callable.  Returns name -> {ms, rounds, reps_per_round, window_s}."""
    reps = {}
    for name, fn in variants.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        reps[name] = max(3, int(round_s / max(timed(fn, 3) / 3, 1e-6)))
    times = {name: [] for name in variants}
    while min(sum(t) for t in times.values()) < window:
        for name, fn in variants.items():
            times[name].append(timed(fn, reps[name]))
    return {name: {"ms": statistics.median(t) / reps[name] * 1e3, "ms_min": min(t) / reps[name] * 1e3, "ms_max": max(t) / reps[name] * 1e3,
                   "rounds": len(t), "reps_per_round": reps[name], "window_s": sum(t)} for name, t in times.items()}


def optimizer_variants(params):
    lars_hp = dict(lr=1e-6, weight_decay=1e-6, momentum=0.9, trust_coefficient=0.001)
    adam_hp = dict(lr=1e-6, weight_decay=1e-2)
    return {"lars_hip": LARS(copies(params), **lars_hp).step, "adamw_hip": AdamW(copies(params), **adam_hp).step,
            "radam_hip": RAdam(copies(params), **adam_hp).step, "lars_torch_loop": TorchLoopLARS(copies(params), **lars_hp).step,
            "radam_torch_foreach": torch.optim.RAdam(copies(params), foreach=True, **adam_hp).step}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--kg-nodes", type=int, default=130_000)
    ap.add_argument("--kg-edges", type=int, default=8_000_000)
    ap.add_argument("--outcomes", type=int, default=896)
    ap.add_argument("--window", type=float, default=0.6, help="seconds of timed work per variant, at least")
    ap.add_argument("--skip-pretrain-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "optim_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench.py measures on the GPU: none found")
    M.set_precision("bf16x3")
    avail = D.make_masks(a.batch, 0)
    avail[:, 1] = torch.where(avail[:, 1:].all(dim=1), torch.zeros(a.batch, dtype=torch.bool), avail[:, 1])
    batch, bkg = D.make_batch(a.batch, 0, kg_nodes=a.kg_nodes, kg_edges=a.kg_edges, masks=avail)
    torch.manual_seed(0)
    np.random.seed(0)
    sim = SimCLR_NovelDDI(configs.build_model("twosides321", bkg["data"], 8).encoder, dim=128, mlp_dim=512, T=0.1, raw_encoder_output=True).cuda().train()
    fine = configs.build_model("twosides321", bkg["data"], n_outcomes=a.outcomes).cuda()
    out = {"device": torch.cuda.get_device_name(0), "window_s_at_least": a.window, "bytes_per_element": 28, "parameter_sets": {}}
    for name, model in (("simclr_configs2", sim), ("twosides_finetune", fine)):
        params = [p for p in model.parameters()]
        elems = sum(p.numel() for p in params)
        res = alternate(optimizer_variants(params), a.window)
        for r in res.values():
            r["GB_per_s_by_28B_count"] = 28 * elems / (r["ms"] * 1e-3) / 1e9
        out["parameter_sets"][name] = {"tensors": len(params), "tensors_scaled_by_lars": sum(p.ndim > 1 for p in params), "elements": elems,
                                       "chunks": sum(-(-p.numel() // 4096) for p in params), "step": res}
        print(name, json.dumps(out["parameter_sets"][name]), flush=True)
    del fine
    if not a.skip_pretrain_step:
        b = D.batch_to(batch, "cuda")
        kgc = {"data": bkg["data"].to("cuda"), "drug_index_map": bkg["drug_index_map"].cuda()}
        bank = MK.get_pretrain_masks(list(range(a.batch)), avail.numpy().astype(np.int64), "str_center_uni", False, 0.2)
        draw = MK.StrCenterUniSampler(bank)
        data = (b["strs"], kgc, b["cv"], b["tx"])
        steps = {"pretrain_step_adamw": PretrainStep(sim, AdamW(sim.parameters(), lr=1e-6, weight_decay=1e-2)),
                 "pretrain_step_lars": PretrainStep(sim, LARS(sim.parameters(), lr=1e-6, weight_decay=1e-6, momentum=0.9))}

        def one(step):
            def fn():
                m1, m2 = draw(range(a.batch))                   # the host-side view draw of pretrain.py:71, inside the step
                step.step(batch["drugs"], m1, m2, None, data)
            return fn
        out["pretrain_step"] = dict(alternate({k: one(v) for k, v in steps.items()}, a.window, round_s=0.15, warmup=3), batch=a.batch,
                                    kg_nodes=a.kg_nodes, kg_edges=a.kg_edges)
        print("pretrain_step", json.dumps(out["pretrain_step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
