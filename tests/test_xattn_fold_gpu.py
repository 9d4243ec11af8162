"""The x-attn pooling of the fusion transformer through the folded path (TransformerFusion._x_attn_pool_folded: logits from the
kv-norm kernel, one product with the composed weights, ops.xattn_fold_pool) against the K|V block -> pool -> out_proj ->
latent2embed path on the same module, and the two new kernels on their own."""
import pytest
import torch

from helpers import rel_err

pytestmark = pytest.mark.gpu

BOUND = {"f32": 3e-5, "bf16x3": 1e-4, "bf16": 3e-2}
SHIPPED = [   # name, heads, head_dim, ffn, layers, norm_first, agg, bottlenecks, act (configs.SHIPPED)
    ("drugbank163", 8, 64, 256, 2, True, "x-attn", 4, "gelu"),
    ("twosides105", 2, 256, 512, 2, True, "x-attn", 2, "gelu"),
    ("twosides321", 8, 256, 1024, 2, True, "x-attn", 2, "gelu"),
]


@pytest.fixture(scope="module")
def M():
    import madrigal_amd.models as _m
    return _m


def _module(M, case, norm_first=None, seed=43):
    from oracle.params import fill_module
    name, H, dh, ffn, nl, nf, agg, nb, actn = case
    m = M.TransformerFusion(128, nb, nl, H, dh, ffn, 0.3, actn, nf if norm_first is None else norm_first, False, agg)
    fill_module(m, seed)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():                                   # non-trivial norm affines and biases: the fold must carry them
        for ln in (m.x_attn_kv_norm, m.x_attn_query_norm):
            ln.weight.copy_(1.0 + 0.3 * torch.randn(ln.weight.shape, generator=g))
            ln.bias.copy_(0.2 * torch.randn(ln.bias.shape, generator=g))
        m.x_attn_mha_layer.in_proj_bias.copy_(0.5 * torch.randn(m.x_attn_mha_layer.in_proj_bias.shape, generator=g))
        m.x_attn_mha_layer.in_proj_weight[:m.latent_dim].mul_(4.0)     # wider logits than the default init gives
    return m.cuda().eval()


def _inputs(m, n, seed=7):
    from madrigal_amd.data import NUM_NON_TX_MODALITIES
    S, nb = m.x_attn_key_padding_mask.shape[1], m.num_tx_bottlenecks
    g = torch.Generator().manual_seed(seed)
    seq = torch.randn(n, S, 128, generator=g) + 0.5
    kpm = torch.rand(n, S, generator=g) < 0.6
    kpm[:, NUM_NON_TX_MODALITIES:NUM_NON_TX_MODALITIES + nb] = False
    return seq.cuda(), kpm.cuda()


def _run(M, m, seq, kpm, prec, live, fold):
    m.compose_pool = fold
    with torch.no_grad(), M.precision(prec):
        if live:
            plan = m.live_token_plan(kpm, None)
            tokens = seq.reshape(-1, 128).index_select(0, plan["token_index"]).contiguous()
            return m.forward_tokens(tokens, plan).cpu()
        return m(seq, kpm).cpu()


def _folded_entries(m):
    return [k for k in m.__dict__.get("_mdg_derived", {}) if k[0] == "x_attn_fold"]


@pytest.mark.parametrize("live", [True, False], ids=["live", "dense"])
@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("case", SHIPPED, ids=[c[0] for c in SHIPPED])
def test_folded_pool_matches_unfolded(M, case, prec, live):
    m = _module(M, case)
    seq, kpm = _inputs(m, 384)
    want = _run(M, m, seq, kpm, prec, live, False)
    assert not _folded_entries(m)
    got = _run(M, m, seq, kpm, prec, live, True)
    assert _folded_entries(m) == [("x_attn_fold", prec)]              # the folded path really ran
    assert torch.isfinite(got).all()
    assert rel_err(got, want) <= BOUND[prec]


def test_post_norm_and_hooked_modules_take_the_unfolded_path(M):
    m = _module(M, SHIPPED[0], norm_first=False)
    seq, kpm = _inputs(m, 200)
    for live in (True, False):
        assert torch.equal(_run(M, m, seq, kpm, "bf16x3", live, True), _run(M, m, seq, kpm, "bf16x3", live, False))
    assert not _folded_entries(m)
    m = _module(M, SHIPPED[0])
    m.x_attn_mha_layer.register_forward_hook(lambda *a: None)
    for live in (True, False):
        assert torch.equal(_run(M, m, seq, kpm, "bf16x3", live, True), _run(M, m, seq, kpm, "bf16x3", live, False))
    assert not _folded_entries(m)


def test_fold_follows_in_place_parameter_changes(M):
    """C, G, c_z and C's image are cached on the module: an in-place change of any source parameter rebuilds them."""
    m = _module(M, SHIPPED[0])
    seq, kpm = _inputs(m, 128)
    mha, qn = m.x_attn_mha_layer, m.x_attn_query_norm
    before = _run(M, m, seq, kpm, "bf16x3", True, True)
    for p in (m.x_attn_query, qn.weight, qn.bias, mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias,
              m.latent2embed.weight, m.latent2embed.bias):
        with torch.no_grad():                               # not a scaling or a shift: LN_q would undo those on the query
            p.mul_(1.25).add_(0.1 * torch.linspace(-1.0, 1.0, p.numel(), device=p.device).reshape(p.shape))
        got = _run(M, m, seq, kpm, "bf16x3", True, True)
        assert rel_err(got, before) > 1e-4, p.shape
        assert rel_err(got, _run(M, m, seq, kpm, "bf16x3", True, False)) <= BOUND["bf16x3"]
        before = got


@pytest.mark.parametrize("n", [1, 333])
@pytest.mark.parametrize("Tk,H", [(2, 8), (4, 2), (1, 8)])
def test_fold_pool_kernel_against_fp64(n, Tk, H):
    from madrigal_amd import ops
    D = 128
    g = torch.Generator().manual_seed(n + Tk + H)
    P = torch.randn(n * Tk, H * D, generator=g)
    logits = torch.randn(n * Tk, H, generator=g) * 30.0
    c_z = torch.randn(D, generator=g)
    z = ops.xattn_fold_pool(P.cuda(), logits.cuda(), c_z.cuda(), n, Tk)
    a = torch.softmax(logits.double().reshape(n, Tk, H), dim=1)
    want = (a.unsqueeze(-1) * P.double().reshape(n, Tk, H, D)).sum((1, 2)) + c_z.double()
    assert z.shape == (n, D)
    assert rel_err(z.cpu(), want) <= 1e-6
    for _ in range(3):                                                # fixed summation order: equal bits launch after launch
        assert torch.equal(ops.xattn_fold_pool(P.cuda(), logits.cuda(), c_z.cuda(), n, Tk), z)


def test_fold_pool_validates_its_arguments():
    from madrigal_amd import ops
    P, lg, cz = torch.zeros(8, 256, device="cuda"), torch.zeros(8, 2, device="cuda"), torch.zeros(128, device="cuda")
    with pytest.raises(ValueError):
        ops.xattn_fold_pool(P, lg, cz, 3, 2)                           # rows != n * Tk
    with pytest.raises(ValueError):
        ops.xattn_fold_pool(P.double(), lg, cz, 4, 2)
    with pytest.raises(ValueError):
        ops.xattn_fold_pool(P.cpu(), lg, cz, 4, 2)


@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("d,H", [(512, 8), (512, 2), (2048, 8)])
def test_norm_logits_against_fp64_and_norm_unchanged(prec, d, H):
    """The logits are the dot products of the normalised fp32 rows with G; the rows and image are layernorm_packed's bit for bit."""
    from madrigal_amd import ops
    g = torch.Generator().manual_seed(d + H)
    x = (torch.randn(1001, d, generator=g) * 3 + 1).cuda()
    w, b = (1.0 + 0.3 * torch.randn(d, generator=g)).cuda(), (0.2 * torch.randn(d, generator=g)).cuda()
    G = torch.randn(H, d, generator=g).cuda()
    with torch.no_grad():
        y, img, logits = ops.layernorm_logits(x, w, b, 1e-5, G, prec)
        y0, img0 = ops.layernorm_packed(x, w, b, 1e-5, prec, want_fp32=True)
        y1, img1 = ops.layernorm_packed(x, w, b, 1e-5, prec, want_fp32=False)
    assert logits.shape == (1001, H)
    if prec == "f32":
        assert img is None and img0 is None and torch.equal(y, y0)
    else:
        assert y is None and y1 is None and torch.equal(img, img0) and torch.equal(img, img1)
    ref = y0.double() @ G.double().T
    assert rel_err(logits.cpu(), ref.cpu()) <= 1e-5
    with torch.no_grad():
        again = ops.layernorm_logits(x, w, b, 1e-5, G, prec)[2]
    assert torch.equal(again, logits)
