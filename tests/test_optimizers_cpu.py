"""CPU checks of the LARS / RAdam path: the C ABI is declared and exported, the float64 restatement of LARS that the GPU test is
measured against (tests/lars_ref.py) agrees with the reference's own fp32 run (tests/golden/lars_reference.npz, recorded by
scripts/gen_optim_golden.py from madrigal/utils.py:628-662), and the factories build the reference's optimizers."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lars_ref as R                                             # noqa: E402


def test_optimizer_symbols_are_declared_and_exported():
    from madrigal_amd import _lib
    syms = _lib.declared_symbols()
    L = _lib.lib()
    for s in ("mdg_lars_multi", "mdg_lars_multi_workspace_bytes", "mdg_radam_multi", "mdg_adamw_multi"):
        assert s in syms and hasattr(L, s), s
    assert L.mdg_abi_version() >= 12


def test_lars_workspace_query_and_argument_checks_need_no_gpu():
    from madrigal_amd._lib import lib
    L, c = lib(), ctypes.c_int64
    assert L.mdg_lars_multi_workspace_bytes(c(0), c(0)) == 0
    # a pair of floats per chunk, one float per tensor
    assert L.mdg_lars_multi_workspace_bytes(c(300), c(7)) >= 300 * 8 + 7 * 4
    assert L.mdg_lars_multi_workspace_bytes(c(301), c(7)) >= L.mdg_lars_multi_workspace_bytes(c(300), c(7))
    # the entry points validate before they touch the device
    z = ctypes.c_size_t(0)
    assert L.mdg_lars_multi(None, None, None, None, None, None, c(0), c(0), None, z, None) == 0
    assert L.mdg_lars_multi(None, None, None, None, None, None, c(-1), c(0), None, z, None) == -1
    assert L.mdg_lars_multi(None, None, None, None, None, None, c(4), c(5), None, z, None) == -1 and b"tensor count" in L.mdg_last_error()
    assert L.mdg_lars_multi(None, None, None, None, None, None, c(4), c(2), None, z, None) == -1 and b"null table" in L.mdg_last_error()
    assert L.mdg_radam_multi(None, None, None, None, c(0), None) == 0
    assert L.mdg_radam_multi(None, None, None, None, c(3), None) == -1 and b"null table" in L.mdg_last_error()


def test_float64_restatement_of_lars_agrees_with_the_reference_run(golden):
    """The bound is twice the distance the generator recorded between the reference's fp32 run and its float64 run (the reference's
    fp32 ``torch.norm`` is that far from exact; the factor 2 covers another CPU thread count re-ordering torch's sums)."""
    g = golden("lars_reference")
    assert int(g["steps"]) == R.STEPS and int(g["param_seed"]) == R.PARAM_SEED
    assert [int(s) for s in g["stride"]] == [R.STRIDE.get(i, 1) for i in range(len(R.SHAPES))]
    assert g["grad_seeds"].tolist() == [[100 * s + i for i in range(len(R.SHAPES))] for s in range(R.STEPS)]
    ps, mus = R.restatement()
    for i in range(len(R.SHAPES)):
        for name, mine, bound in (("p", ps[i], float(g["worst_p"])), ("mu", mus[i], float(g["worst_mu"]))):
            d = R.distance(R.stored(i, mine), g[f"{name}_{i}"])
            print(f"tensor {i} {name}: {d:.3e} (bound {2 * bound:.3e})")
            assert d <= 2 * bound, (i, name, d, bound)
    assert 0 < float(g["worst_p"]) < 1e-5 and 0 < float(g["worst_mu"]) < 1e-5      # fp32 rounding, not a different algorithm
    # the zero parameter stayed put while its gradient was zero, and moved afterwards (q = 1 on both sides of the switch)
    assert float(mus[R.ZERO_PARAM].abs().max()) > 0
    R.restatement.cache_clear()
    p2, mu2 = R.restatement(2)
    assert not p2[R.ZERO_PARAM].any() and not mu2[R.ZERO_PARAM].any()
    R.restatement.cache_clear()


def test_lars_state_layout_is_the_references(golden):
    from madrigal_amd.optim import LARS
    g = golden("lars_reference")
    assert {str(k) for k in g["state_keys"]} == {"mu"}
    assert int(g["n_state"]) == len(R.SHAPES)
    opt = LARS(R.param_groups([torch.nn.Parameter(p) for p in R.initial_params()]), **R.DEFAULTS)
    sd = opt.state_dict()
    assert sorted(k for k in sd["param_groups"][0] if k != "params") == [str(k) for k in g["group_keys"]]
    assert [grp["trust_coefficient"] for grp in sd["param_groups"]] == [0.001, 0.3, 0.001]
    assert [grp["momentum"] for grp in sd["param_groups"]] == [0.9, 0.5, 0.9]
    d = LARS([torch.nn.Parameter(torch.zeros(2))]).defaults                        # the reference's defaults
    assert d == dict(lr=0, weight_decay=0, momentum=0.9, trust_coefficient=0.001)
    # a state in the reference's layout loads
    sd["state"] = {i: {"mu": torch.from_numpy(g[f"mu_{i}"].copy()).reshape(R.SHAPES[i])} for i in range(len(R.SHAPES)) if i not in R.STRIDE}
    opt.load_state_dict(sd)
    assert all(set(st) == {"mu"} for st in opt.state.values()) and len(opt.state) == len(R.SHAPES) - len(R.STRIDE)


def test_steps_refuse_cpu_parameters():
    from madrigal_amd.optim import LARS, RAdam
    for cls in (LARS, RAdam):
        p = torch.nn.Parameter(torch.zeros(4, 4))
        p.grad = torch.ones(4, 4)
        with pytest.raises(RuntimeError, match="on the GPU only"):
            cls([p], lr=0.1).step()
    with pytest.raises(ValueError):
        RAdam([torch.nn.Parameter(torch.zeros(2))], betas=(1.0, 0.9))


@pytest.fixture(scope="module")
def small_model():
    from test_checkpoint_cpu import _build
    from madrigal_amd import data as D
    _, bkg = D.make_batch(12, 3, kg_nodes=200, kg_edges=900)
    torch.manual_seed(0)
    return _build(bkg["data"])


HP = dict(structure_encoder_lr=1e-3, kg_encoder_lr=2e-3, perturb_encoders_lr=3e-3, fusion_lr=4e-3, decoder_lr=5e-3, wd=1e-2, beta1=0.8,
          beta2=0.98, eps=1e-7)


def test_create_optimizer_builds_radam_over_the_same_groups(small_model):
    from madrigal_amd import optim
    model, _ = small_model
    a = optim.create_optimizer(model, dict(HP, optimizer="adamw"))
    r = optim.create_optimizer(model, dict(HP, optimizer="radam"))
    assert type(a) is optim.AdamW and type(r) is optim.RAdam and type(optim.create_optimizer(model, HP)) is optim.AdamW
    assert len(a.param_groups) == len(r.param_groups) > 2
    for ga, gr in zip(a.param_groups, r.param_groups):
        assert all(x is y for x, y in zip(ga["params"], gr["params"])) and len(ga["params"]) == len(gr["params"])
        assert (gr["lr"], gr["weight_decay"], gr["betas"], gr["eps"]) == (ga["lr"], ga["weight_decay"], (0.8, 0.98), 1e-7)
        assert gr["decoupled_weight_decay"] is False                              # torch.optim.RAdam's default: L2
    ref = torch.optim.RAdam(optim.parameter_groups(model, HP), betas=(0.8, 0.98), eps=1e-7)
    assert set(r.state_dict()["param_groups"][0]) <= set(ref.state_dict()["param_groups"][0])
    for name in ("sgd", "adafactor", "lars"):
        with pytest.raises(NotImplementedError):
            optim.create_optimizer(model, dict(HP, optimizer=name))


def test_create_pretrain_optimizer_and_checkpoint_take_lars(small_model, tmp_path):
    """pretrain.py:175-178, and the file of pretrain.py:230-236 with a LARS state in it."""
    from madrigal_amd import checkpoint as CK, optim
    from madrigal_amd.simclr import SimCLR_NovelDDI
    model, cfg = small_model
    sim = SimCLR_NovelDDI(model.encoder, dim=128, mlp_dim=64, T=0.1, raw_encoder_output=True)
    hp = dict(pretrain_lr=0.3 * 2048 / 512, pretrain_wd=1e-6, pretrain_momentum=0.8, pretrain_eps=1e-7, pretrain_beta1=0.85)
    lars = optim.create_pretrain_optimizer(sim, hp, "lars")
    assert type(lars) is optim.LARS and len(lars.param_groups) == 1
    assert len(lars.param_groups[0]["params"]) == len(list(sim.parameters()))
    assert {k: v for k, v in lars.param_groups[0].items() if k in lars.defaults} == dict(lr=1.2, weight_decay=1e-6, momentum=0.8, trust_coefficient=0.001)
    adamw = optim.create_pretrain_optimizer(sim, hp, "adamw")
    grp = adamw.param_groups[0]
    assert type(adamw) is optim.AdamW and (grp["lr"], grp["weight_decay"], grp["eps"], grp["betas"]) == (1.2, 1e-6, 1e-7, (0.85, 0.999))
    with pytest.raises(NotImplementedError):
        optim.create_pretrain_optimizer(sim, hp, "sgd")
    path = str(tmp_path / "checkpoint_0.pt")
    CK.save_pretrain_checkpoint(path, sim, lars, epoch=1, encoder_configs=cfg, kg_args={"kg_sampling_num_neighbors": None})
    raw = torch.load(path, map_location="cpu", weights_only=False)
    assert raw["optimizer"]["param_groups"][0]["trust_coefficient"] == 0.001 and raw["optimizer"]["state"] == {}
    fresh = optim.create_pretrain_optimizer(sim, hp, "lars")
    fresh.load_state_dict(raw["optimizer"])
