"""LARS and RAdam on the HIP path (madrigal_amd.optim, mdg_lars_multi / mdg_radam_multi).

LARS is measured against the float64 restatement of tests/lars_ref.py (which tests/test_optimizers_cpu.py ties to the reference's own
run): the reference's fp32 run is itself 2e-6 .. 4e-6 away from exact on the large tensors (its fp32 ``torch.norm``), so it cannot be
the yardstick of a 2e-6 bound.  RAdam is measured against ``torch.optim.RAdam`` on float64 CPU copies.  The bound is that of the
project's AdamW unit test, 2e-6 under its ``_close`` measure: fp32 partial sums of 4096 elements, summed in double per tensor, stay
at or below about 5e-7 on these inputs."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lars_ref as R                                             # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 2e-6


def _close(a, b, tol, what):
    err = R.distance(a, b)
    print(f"{what}: {err:.3e}")
    assert err <= tol, f"{what}: rel err {err:.3e} > {tol}"


def _run_lars(steps=R.STEPS, offset=None):
    """The input set of tests/lars_ref.py through optim.LARS.  ``offset``: the parameters are views that start that many floats into
    a 16-byte aligned buffer."""
    from madrigal_amd.optim import LARS
    ps = []
    for p in R.initial_params():
        if offset:
            buf = torch.zeros(p.numel() + offset, device=DEV)
            buf[offset:] = p.reshape(-1).to(DEV)
            p = buf[offset:].view(p.shape)
            assert p.data_ptr() % 16 == 4 * offset
        ps.append(torch.nn.Parameter(p.to(DEV)))
    opt = LARS(R.param_groups(ps), **R.DEFAULTS)
    for s in range(steps):
        for i, p in enumerate(ps):
            g = R.grad(s, i)
            p.grad = None if g is None else g.to(DEV)
        opt.step()
    return ps, opt


@pytest.fixture(scope="module")
def lars_run():
    ps, opt = _run_lars()
    return ps, opt, copy.deepcopy(opt.state_dict()), [p.detach().clone() for p in ps]


def test_lars_matches_the_float64_restatement(lars_run):
    ps, opt, _, p_end = lars_run
    ref_p, ref_mu = R.restatement()
    for i, p in enumerate(ps):
        _close(p_end[i], ref_p[i], TOL, f"tensor {i} {R.SHAPES[i]} p")
        _close(opt.state[p]["mu"], ref_mu[i], TOL, f"tensor {i} {R.SHAPES[i]} mu")
        assert set(opt.state[p]) == {"mu"}
    # group B moved by more than its own norm: an error in q could not hide behind p
    p0 = R.initial_params()
    assert float((p_end[8].cpu() - p0[8]).norm() / p0[8].norm()) > 1.0


def test_lars_leaves_one_dimensional_tensors_unscaled(lars_run):
    """No weight decay and no trust ratio: ``mu`` is the plain momentum recursion of the gradients, to the bit."""
    ps, opt, _, _ = lars_run
    for i, shape in enumerate(R.SHAPES):
        if len(shape) != 1:
            continue
        mu = torch.zeros(shape)
        for s in range(R.STEPS):
            mu = mu * R.hyper(i)["momentum"] + R.grad(s, i)
        assert torch.equal(opt.state[ps[i]]["mu"].cpu(), mu), i


def test_lars_is_reproducible_and_independent_of_alignment(lars_run):
    _, opt, _, p_end = lars_run
    again, opt2 = _run_lars()
    shifted, opt3 = _run_lars(offset=1)                             # every access 4-byte: same sums in the same order
    for a, b, c in zip(p_end, again, shifted):
        assert torch.equal(a, b) and torch.equal(a, c)
    for (x, y, z) in zip(opt.state.values(), opt2.state.values(), opt3.state.values()):
        assert torch.equal(x["mu"], y["mu"]) and torch.equal(x["mu"], z["mu"])


def test_lars_bumps_version_counters():
    from madrigal_amd.optim import LARS
    p = torch.nn.Parameter(torch.ones(5, 5, device=DEV))
    opt = LARS([p], lr=0.1)
    p.grad = torch.ones_like(p)
    opt.step()
    v_p, v_mu = p._version, opt.state[p]["mu"]._version
    opt.step()
    assert p._version > v_p and opt.state[p]["mu"]._version > v_mu


def test_lars_resumes_bit_identically_and_loads_the_reference_layout(lars_run, golden):
    """Resume over the whole input set, then a state dict in the reference's layout.  The fixture holds the two large tensors as
    every 37th / 61st element only (file size), so the reference-layout part loads the nine tensors stored whole: none of them has
    more than three chunks.  The many-chunk tensors go through the main run and the bit-identical resume above it."""
    from madrigal_amd.optim import LARS
    ps, opt, sd, p_end = lars_run
    fresh_p = [torch.nn.Parameter(p.clone()) for p in p_end]
    cont_p = [torch.nn.Parameter(p.clone()) for p in p_end]
    fresh, cont = LARS(R.param_groups(fresh_p), **R.DEFAULTS), LARS(R.param_groups(cont_p), **R.DEFAULTS)
    fresh.load_state_dict(copy.deepcopy(sd))
    for p, q in zip(cont_p, ps):                                    # the original's state, continued without a state_dict round trip
        cont.state[p]["mu"] = opt.state[q]["mu"].clone()
    for i in range(len(ps)):
        g = R.grad(R.STEPS, i).to(DEV)
        fresh_p[i].grad, cont_p[i].grad = g.clone(), g.clone()
    fresh.step()
    cont.step()
    for a, b in zip(fresh_p, cont_p):
        assert torch.equal(a, b) and torch.equal(fresh.state[a]["mu"], cont.state[b]["mu"])
    # a state dict as the reference writes it: its parameters and its ``mu`` (every tensor the fixture holds whole), one more step
    g = golden("lars_reference")
    keep = [i for i in range(len(R.SHAPES)) if i not in R.STRIDE]
    rp = [torch.nn.Parameter(torch.from_numpy(g[f"p_{i}"].copy()).reshape(R.SHAPES[i]).to(DEV)) for i in keep]
    ropt = LARS([dict(params=[rp[k]], **R.hyper(i)) for k, i in enumerate(keep)])
    ref_sd = ropt.state_dict()
    ref_sd["state"] = {k: {"mu": torch.from_numpy(g[f"mu_{i}"].copy()).reshape(R.SHAPES[i])} for k, i in enumerate(keep)}
    ropt.load_state_dict(ref_sd)
    for k, i in enumerate(keep):
        rp[k].grad = R.grad(R.STEPS, i).to(DEV)
    ropt.step()
    for k, i in enumerate(keep):
        want_p, want_mu = R.lars_update(torch.from_numpy(g[f"p_{i}"]).double().reshape(R.SHAPES[i]), R.grad(R.STEPS, i, torch.float64),
                                        torch.from_numpy(g[f"mu_{i}"]).double().reshape(R.SHAPES[i]), **R.hyper(i))
        _close(rp[k], want_p, TOL, f"resumed from the reference's state: tensor {i} p")
        _close(ropt.state[rp[k]]["mu"], want_mu, TOL, f"resumed from the reference's state: tensor {i} mu")


class _TorchLARS(torch.optim.Optimizer):
    """The same algorithm in torch ops over whatever gradients the step left (float64 arithmetic, fp32 storage)."""

    def __init__(self, params, **kw):
        super().__init__(params, dict(kw))

    @torch.no_grad()
    def step(self):
        for grp in self.param_groups:
            for p in grp["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                mu = st["mu"] if "mu" in st else torch.zeros_like(p)
                new_p, new_mu = R.lars_update(p.double(), p.grad.double(), mu.double(), grp["lr"], grp["weight_decay"], grp["momentum"],
                                              grp["trust_coefficient"])
                st["mu"] = new_mu.float()
                p.copy_(new_p.float())


def test_lars_in_the_pretraining_loop():
    """pretrain.py's loop with ``--pretrain_optimizer lars`` on the 96-drug fixture of test_pretrain_gpu: the loss falls, a seeded run
    repeats bit for bit, and ONE step from identical weights equals the same step taken with a torch-op LARS over the HIP gradients
    (later steps would compare two diverging trajectories, not the kernel)."""
    from madrigal_amd import data as D, masks as MK, models as M
    from madrigal_amd.optim import LARS
    from madrigal_amd.train import PretrainStep
    from test_pretrain_gpu import _build, _views
    n, seed = 96, 12
    hp = dict(lr=0.5, weight_decay=1e-6, momentum=0.9, trust_coefficient=0.02)

    def run(steps, cls):
        torch.manual_seed(seed)
        np.random.seed(seed)
        avail, _, _ = _views(n, seed)
        batch, bkg = D.make_batch(n, seed, kg_nodes=600, kg_edges=6000, masks=avail)
        model = _build(M, bkg["data"], False, True, mlp_dim=256, T=0.5).cuda().train()
        bank = MK.get_pretrain_masks(list(range(n)), avail.numpy().astype(np.int64), "str_center_uni", False, 0.2)
        b = D.batch_to(batch, "cuda")
        kgc = {"data": bkg["data"].to("cuda"), "drug_index_map": bkg["drug_index_map"].cuda()}
        opt = cls(model.parameters(), **hp)
        step = PretrainStep(model, opt)
        losses = []
        for _ in range(steps):
            m1, m2 = MK.pretrain_modality_subset_sampler([bank[d] for d in range(n)], "str_center_uni", False)
            losses.append(float(step.step(b["drugs"], m1.cuda(), m2.cuda(), None, (b["strs"], kgc, b["cv"], b["tx"]))))
        return losses, model, opt
    l1, m1_, _ = run(10, LARS)
    l2, m2_, _ = run(10, LARS)
    print("losses under LARS:", l1)
    assert all(np.isfinite(l1)) and min(l1[-3:]) < l1[0], l1
    assert l1 == l2
    assert all(torch.equal(a, b) for a, b in zip(m1_.parameters(), m2_.parameters()))
    la, ma, oa = run(1, LARS)
    lb, mb, ob = run(1, _TorchLARS)
    assert la == lb
    n_scaled = 0
    for (name, a), b in zip(ma.named_parameters(), mb.parameters()):
        assert (a.grad is None) == (b.grad is None), name
        if a.grad is None:
            assert torch.equal(a, b) and a not in oa.state, name
            continue
        assert torch.equal(a.grad, b.grad), name
        n_scaled += a.ndim > 1
        _close(a, b, TOL, f"{name} after one step")
        _close(oa.state[a]["mu"], ob.state[b]["mu"], TOL, f"{name} mu after one step")
    assert n_scaled > 20, n_scaled


@pytest.mark.parametrize("decoupled", [False, True], ids=["l2", "decoupled"])
def test_radam_matches_torch_optim_over_param_groups(decoupled):
    """The AdamW unit test's shapes and groups; betas (0.9, 0.98): rho_t passes 5 at t = 6, so steps 1-5 take the unrectified branch
    and 6-8 the rectified one, one step later for the parameter that skips the second step."""
    from madrigal_amd.optim import RAdam
    torch.manual_seed(0)
    shapes = [(3,), (128, 130), (5000,), (64, 64, 3), (1,)]
    ref_p = [torch.nn.Parameter(torch.randn(s).double()) for s in shapes]
    my_p = [torch.nn.Parameter(p.detach().float().to(DEV)) for p in ref_p]

    def groups(ps):
        return [{"params": ps[:2], "lr": 1e-2, "weight_decay": 0.0}, {"params": ps[2:], "lr": 3e-3, "weight_decay": 0.1}]
    kw = dict(betas=(0.9, 0.98), eps=1e-6, decoupled_weight_decay=decoupled)
    ref = torch.optim.RAdam(groups(ref_p), **kw)
    mine = RAdam(groups(my_p), **kw)
    assert [h[6] > 0 for h in (mine._hyper(mine.param_groups[0], k) for k in range(1, 9))] == [False] * 5 + [True] * 3
    sched_r = torch.optim.lr_scheduler.StepLR(ref, 3, 0.5)
    sched_m = torch.optim.lr_scheduler.StepLR(mine, 3, 0.5)

    def set_grads(it, lists, skip):
        for i in range(len(shapes)):
            g = None if skip and i == 4 else torch.randn(shapes[i], generator=torch.Generator().manual_seed(100 * it + i))
            for ps in lists:
                ps[i].grad = None if g is None else g.to(device=ps[i].device, dtype=ps[i].dtype)
    for it in range(8):
        set_grads(it, (ref_p, my_p), skip=it == 1)
        ref.step()
        mine.step()
        sched_r.step()
        sched_m.step()
        for i, (a, b) in enumerate(zip(ref_p, my_p)):
            _close(b, a, TOL, f"radam step {it + 1} parameter {i}")
    sd, ref_sd = mine.state_dict(), ref.state_dict()
    for i in range(5):
        assert set(sd["state"][i].keys()) == set(ref_sd["state"][i].keys()) == {"step", "exp_avg", "exp_avg_sq"}
        _close(sd["state"][i]["exp_avg"], ref_sd["state"][i]["exp_avg"], TOL, f"exp_avg {i}")
        _close(sd["state"][i]["exp_avg_sq"], ref_sd["state"][i]["exp_avg_sq"], TOL, f"exp_avg_sq {i}")
    assert [float(sd["state"][i]["step"]) for i in range(5)] == [float(ref_sd["state"][i]["step"]) for i in range(5)] == [8, 8, 8, 8, 7]
    assert set(sd["param_groups"][0]) <= set(ref_sd["param_groups"][0])
    # resume: a fresh optimizer loaded from the state continues exactly like the original (step counts included)
    fresh_p = [torch.nn.Parameter(p.detach().clone()) for p in my_p]
    fresh = RAdam(groups(fresh_p), **kw)
    fresh.load_state_dict(copy.deepcopy(sd))
    set_grads(9, (ref_p, my_p, fresh_p), skip=False)
    ref.step()
    mine.step()
    fresh.step()
    for a, b, c in zip(ref_p, my_p, fresh_p):
        _close(b, a, TOL, "radam parameter after 9 steps")
        assert torch.equal(b, c)
    assert float(fresh.state_dict()["state"][4]["step"]) == 8.0


@pytest.mark.parametrize("name", ["LARS", "RAdam"])
def test_refusals(name):
    from madrigal_amd import optim
    cls = getattr(optim, name)

    def one(p, g):
        p = torch.nn.Parameter(p)
        p.grad = g
        return cls([p], lr=0.1)
    with pytest.raises(RuntimeError, match="GPU only"):
        one(torch.zeros(4, 4), torch.ones(4, 4)).step()
    with pytest.raises(RuntimeError, match="fp32"):
        one(torch.zeros(4, 4, device=DEV, dtype=torch.float64), torch.ones(4, 4, device=DEV, dtype=torch.float64)).step()
    with pytest.raises(RuntimeError, match="dense"):
        one(torch.zeros(4, 4, device=DEV), torch.ones(4, 4, device=DEV).to_sparse()).step()
    with pytest.raises(RuntimeError, match="contiguous"):
        one(torch.zeros(4, 6, device=DEV).t(), torch.ones(6, 4, device=DEV)).step()
    ok = one(torch.zeros(4, 4, device=DEV), None)                    # a parameter without a gradient is skipped, not refused
    ok.step()
    assert len(ok.state) == 0
