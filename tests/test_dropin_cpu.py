"""The drop-in boundary as the reference's own factory and optimizer builder see it (CPU, construction only).  What the
reference's get_model and create_optimizer produced over the aliased classes is recorded in tests/golden/dropin.npz by
oracle/check_dropin.py --write-golden; the test rebuilds every model from the recorded config dicts and checks it
against that record."""
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adaptor_and_encoder_are_sibling_classes():
    """The reference's create_optimizer (madrigal/utils.py:467-479) tells the fusion-side adaptors from the tabular encoders
    with isinstance(): MLPAdaptor must not be an MLPEncoder (nor the other way round), as in the reference (models.py:121, :459)."""
    from madrigal_amd import models as M
    assert not issubclass(M.MLPAdaptor, M.MLPEncoder) and not issubclass(M.MLPEncoder, M.MLPAdaptor)
    a, e = M.MLPAdaptor(8, [8], 4, 0.0, "ln", "relu"), M.MLPEncoder(8, [8], 4, 0.0, None, "relu")
    assert sorted(a.state_dict()) == sorted(e.state_dict())


def test_reference_get_model_and_create_optimizer_over_the_aliased_classes(golden):
    """Per recorded case (two fixture cases and the shipped hardy_sweep_321 yaml): the model built from the config dicts the
    reference's get_model returned has the factory's module classes and parameter names in its order, every parameter sits in
    the (lr, weight decay) group the reference's create_optimizer put it in (the learned tokens in none), and the fixture
    cases' names and groups equal the reference's own model's (param_groups.npz)."""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    from check_dropin import dropin_kg, groups_by_name
    from madrigal_amd import models as AM
    from madrigal_amd.optim import parameter_groups
    g, own = golden("dropin"), golden("param_groups")
    _, bkg = dropin_kg()
    for case in [str(c) for c in g["cases"]]:
        enc_cfg, model_cfg = json.loads(str(g[case + "_enc_cfg"])), json.loads(str(g[case + "_model_cfg"]))
        model = AM.NovelDDIMultilabel(AM.NovelDDIEncoder(all_kg_data=bkg["data"], **enc_cfg), **model_cfg)
        modules = [f"{n}={type(m).__module__}.{type(m).__qualname__}" for n, m in model.named_modules()]
        assert modules == [str(s) for s in g[case + "_modules"]], case
        assert all(s.split("=", 1)[1].startswith(("madrigal_amd.", "torch.nn.")) for s in modules), case
        names = [k for k, _ in model.named_parameters()]
        assert names == [str(k) for k in g[case + "_names"]], case
        groups = parameter_groups(model, json.loads(str(g[case + "_opt_hp"])))
        assert len(groups) == int(g[case + "_n_groups"]), case
        got = groups_by_name(model, groups)
        for k, (lr, wd) in zip(names, g[case + "_lr_wd"]):
            if math.isnan(lr):
                assert k not in got, (case, k)                   # cls / tx_bottleneck_tokens: in no group
            else:
                assert got[k] == (lr, wd), (case, k, got.get(k), (lr, wd))
        if case + "_names" in own.files:
            assert sorted(names) == sorted(str(k) for k in own[case + "_names"]), case
            want = {str(k): tuple(v) for k, v in zip(own[case + "_names"], own[case + "_lr_wd"])}
            assert all(got[k] == v for k, v in want.items() if not math.isnan(v[0])), case
        if case == "hardy321":
            assert len(got) == len(names) - 1                      # tx_bottleneck_tokens left out
            assert model.encoder.transformer.embed2latent.weight.shape[0] == 2048
            assert model.decoder.parametrizations.weight.original.shape == (896, 128, 128)
        again = AM.NovelDDIMultilabel(AM.NovelDDIEncoder(all_kg_data=bkg["data"], **enc_cfg), **model_cfg)
        again.load_state_dict(model.state_dict())                 # checkpoint interop through the reference's config dicts
