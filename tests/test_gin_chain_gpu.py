"""GraphIsomorphismNetwork in inference with each layer's dense chain as one launch (``fuse_layer_chain``) against the same
module with one dense block per launch: bit-equal outputs, the old path where the chain does not apply, cache invalidation."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    import madrigal_amd.models as _m
    return _m


@pytest.fixture(scope="module")
def mols():
    """7 drugs; every bond of one atom in the middle of the batch removed (an atom without bonds)."""
    from madrigal_amd import data as D
    b = D.make_molecules(7, seed=11)
    lone = b.num_node // 2
    keep = (b.edge_list[:, 0] != lone) & (b.edge_list[:, 1] != lone)
    assert 0 < int(keep.sum()) < b.num_edge
    return D.MoleculeBatch(b.node_feature, b.edge_list[keep], b.edge_feature[keep], b.node2graph, b.batch_size, b.edge_weight[keep]).cuda()


def _gin(M, hidden=None, edge_dim="config", seed=3):
    from madrigal_amd.configs import GIN
    from oracle.params import fill_module
    m = M.GraphIsomorphismNetwork(input_dim=67, hidden_dims=(GIN["gin_hidden_dims"] + [128]) if hidden is None else hidden,
                                  edge_input_dim=GIN["gin_edge_input_dim"] if edge_dim == "config" else edge_dim,
                                  num_mlp_layer=GIN["gin_num_mlp_layer"], eps=GIN["gin_eps"], batch_norm=GIN["gin_batch_norm"],
                                  activation=GIN["gin_actn"], readout=GIN["gin_readout"])
    fill_module(m, seed, ())
    g = torch.Generator().manual_seed(seed)
    for layer in m.layers:                                         # running statistics that are not the identity
        layer.batch_norm.running_mean.copy_(torch.randn(layer.batch_norm.num_features, generator=g) * 0.1)
        layer.batch_norm.running_var.copy_(torch.rand(layer.batch_norm.num_features, generator=g) + 0.5)
    return m.cuda().eval()


def _run(M, m, mols, prec, fuse, x=None):
    m.fuse_layer_chain = fuse
    with torch.no_grad(), M.precision(prec):
        out = m(mols, mols.node_feature if x is None else x)
    return out["graph_feature"].clone(), out["node_feature"].clone()


@pytest.fixture
def chain_calls(monkeypatch):
    """Number of ops.linear_chain calls made by the code under test."""
    import madrigal_amd.ops as ops
    calls = []
    real = ops.linear_chain

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(ops, "linear_chain", counting)
    return calls


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
def test_fused_equals_unfused(M, mols, chain_calls, prec):
    m = _gin(M)
    g0, n0 = _run(M, m, mols, prec, False)
    assert len(chain_calls) == 0
    g1, n1 = _run(M, m, mols, prec, True)
    assert len(chain_calls) == len(m.layers) == 4                 # one launch per layer
    assert torch.equal(g1, g0) and torch.equal(n1, n0)
    assert torch.isfinite(n1).all() and (n1 > 0).any()


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
def test_other_shapes(M, mols, chain_calls, prec):
    narrow = _gin(M, hidden=[64, 64])                              # width 64: the old path
    g0, n0 = _run(M, narrow, mols, prec, False)
    g1, n1 = _run(M, narrow, mols, prec, True)
    assert len(chain_calls) == 0 and torch.equal(g1, g0) and torch.equal(n1, n0)
    mixed = _gin(M, hidden=[64, 128])                              # layer 1 (64 -> 128) takes the chain, layer 0 does not
    g0, n0 = _run(M, mixed, mols, prec, False)
    g1, n1 = _run(M, mixed, mols, prec, True)
    assert len(chain_calls) == 1 and torch.equal(g1, g0) and torch.equal(n1, n0)
    del chain_calls[:]
    no_edge = _gin(M, edge_dim=None)                               # no edge_linear: the chain without its edge stage
    g0, n0 = _run(M, no_edge, mols, prec, False)
    g1, n1 = _run(M, no_edge, mols, prec, True)
    assert len(chain_calls) == 4 and torch.equal(g1, g0) and torch.equal(n1, n0)


def test_f32_keeps_the_unfused_path(M, mols, chain_calls):
    m = _gin(M)
    g0, n0 = _run(M, m, mols, "f32", False)
    g1, n1 = _run(M, m, mols, "f32", True)
    assert len(chain_calls) == 0 and torch.equal(g1, g0) and torch.equal(n1, n0)


def test_training_and_gradient_paths_never_chain(M, mols, chain_calls):
    base = _gin(M)
    outs = []
    for fuse in (False, True):                                     # train(): BatchNorm batch statistics
        m = copy.deepcopy(base).train()
        m.fuse_layer_chain = fuse
        with M.precision("bf16x3"):
            o = m(mols, mols.node_feature)
        outs.append((o["graph_feature"].detach().clone(), o["node_feature"].detach().clone()))
    assert len(chain_calls) == 0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    outs = []
    for fuse in (False, True):                                     # eval(), but a gradient is wanted for the input
        m = copy.deepcopy(base).eval()
        for p in m.parameters():
            p.requires_grad_(False)
        m.fuse_layer_chain = fuse
        x = mols.node_feature.clone().requires_grad_(True)
        with M.precision("bf16x3"):
            o = m(mols, x)
        assert o["node_feature"].requires_grad
        outs.append((o["graph_feature"].detach().clone(), o["node_feature"].detach().clone()))
    assert len(chain_calls) == 0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
def test_cached_descriptors(M, mols, monkeypatch, prec):
    from madrigal_amd import _lib
    m = _gin(M)
    L = _lib.lib()
    packs = []
    real = L.mdg_pack_operand

    def counting(*a):
        packs.append(1)
        return real(*a)
    monkeypatch.setattr(L, "mdg_pack_operand", counting)
    g1, n1 = _run(M, m, mols, prec, True)
    first = len(packs)
    assert first >= 4 * 4                                           # the weight images were built: 3 MLP + 1 edge per layer
    derived = [dict(layer.edge_linear._mdg_derived) for layer in m.layers] + [dict(layer.batch_norm._mdg_derived) for layer in m.layers]
    g2, n2 = _run(M, m, mols, prec, True)
    assert len(packs) == first                                      # steady state: no pack kernel
    again = [layer.edge_linear._mdg_derived for layer in m.layers] + [layer.batch_norm._mdg_derived for layer in m.layers]
    for a, b in zip(derived, again):                                # ... and no derived tensor rebuilt
        assert a.keys() == b.keys() and all(a[k] is b[k] for k in a)
    assert torch.equal(g2, g1) and torch.equal(n2, n1)
    layer = m.layers[2]
    changes = [lambda: layer.mlp.layers[1].weight.mul_(1.25), lambda: layer.mlp.layers[0].bias.add_(0.05),
               lambda: layer.edge_linear.weight.mul_(0.5), lambda: layer.batch_norm.running_var.mul_(2.0),
               lambda: layer.batch_norm.running_mean.add_(0.1)]
    prev = n1
    for change in changes:                                          # in-place changes reach the next call
        with torch.no_grad():
            change()
        g_f, n_f = _run(M, m, mols, prec, True)
        g_u, n_u = _run(M, m, mols, prec, False)
        assert not torch.equal(n_f, prev)
        assert torch.equal(g_f, g_u) and torch.equal(n_f, n_u)
        prev = n_f
