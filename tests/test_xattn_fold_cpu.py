"""CPU checks of the folded x-attn pooling of the fusion transformer (models.compose_xattn_pool): in fp64, the per-head softmax of
u G^T over each drug's keys applied to u C^T, plus c_z, equals x_attn_kv_norm -> nn.MultiheadAttention (one query) -> + query ->
latent2embed."""
import pytest
import torch

from madrigal_amd.models import compose_xattn_pool

f8 = torch.float64


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _reference(h, n, Tk, query, qn, kvn, mha, le):
    """Eval-mode pre-norm pooling as the reference module computes it (models.py:422-443), in fp64."""
    d = h.shape[1]
    q = torch.nn.functional.layer_norm(query, (d,), *qn)
    u = torch.nn.functional.layer_norm(h, (d,), *kvn).reshape(n, Tk, d)
    o, _ = mha(q.expand(n, 1, d), u, u, need_weights=False)
    return le(o.reshape(n, d) + q), u.reshape(n * Tk, d)


def _case(d, H, Tk, n, seed, spread=60.0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=f8)                     # noqa: E731
    D = 128
    mha = torch.nn.MultiheadAttention(d, H, batch_first=True, dtype=f8).eval()
    le = torch.nn.Linear(d, D, dtype=f8)
    with torch.no_grad():
        mha.in_proj_weight.copy_(r(3 * d, d) / d ** 0.5)
        mha.in_proj_bias.copy_(r(3 * d))                                       # query, key and value biases all non-zero
        mha.out_proj.weight.copy_(r(d, d) / d ** 0.5)
        mha.out_proj.bias.copy_(r(d))
        le.weight.copy_(r(D, d) / d ** 0.5)
        le.bias.copy_(r(D))
    query = r(1, d)
    qn = (1.0 + 0.3 * r(d), 0.2 * r(d), 1e-5)
    kvn = (1.0 + 0.3 * r(d), 0.2 * r(d), 1e-5)
    h = r(n * Tk, d) * 2.0 + 0.5
    with torch.no_grad():                                                      # widen the logits: spread of > 50 within a head
        q = torch.nn.functional.layer_norm(query, (d,), *qn).reshape(-1)
        dh = d // H
        u = torch.nn.functional.layer_norm(h, (d,), *kvn)
        lg = ((u @ mha.in_proj_weight[d:2 * d].T).reshape(-1, H, dh) * (mha.in_proj_weight[:d] @ q + mha.in_proj_bias[:d]).reshape(H, dh)).sum(-1)
        lg = lg.reshape(n, Tk, H) / dh ** 0.5
        s = spread / max(float((lg.max(1).values - lg.min(1).values).max()), 1e-3)
        mha.in_proj_weight[:d].mul_(s)
        mha.in_proj_bias[:d].mul_(s)
    return h, query, qn, kvn, mha, le


@pytest.mark.parametrize("Tk", [1, 2, 4])
@pytest.mark.parametrize("H", [1, 2, 8])
@pytest.mark.parametrize("d", [512, 2048])
def test_fold_matches_ln_mha_out_proj_latent2embed(d, H, Tk):
    n = 24
    h, query, qn, kvn, mha, le = _case(d, H, Tk, n, seed=d + 10 * H + Tk)
    with torch.no_grad():
        want, u = _reference(h, n, Tk, query, qn, kvn, mha, le)
        C, G, c_z = compose_xattn_pool(query, qn, mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias,
                                       le.weight, le.bias, H)
        D = le.weight.shape[0]
        assert C.shape == (H * D, d) and G.shape == (H, d) and c_z.shape == (D,)
        logits = (u @ G.T).reshape(n, Tk, H)
        if Tk > 1:                                                             # the case really has a wide logit spread
            assert float((logits.max(1).values - logits.min(1).values).max()) > 50.0
        a = torch.softmax(logits, dim=1)                                       # over the Tk keys, per head
        P = (u @ C.T).reshape(n, Tk, H, D)
        got = (a.unsqueeze(-1) * P).sum((1, 2)) + c_z
    assert _rel(got, want) <= 1e-12


def test_fold_takes_fp32_parameters_in_fp64():
    """The shipped parameters are fp32: the composite is formed in fp64 all the same."""
    h, query, qn, kvn, mha, le = _case(512, 8, 2, 16, seed=5)
    mha, le = mha.float(), le.float()
    query, qn = query.float(), tuple(t.float() if torch.is_tensor(t) else t for t in qn)
    C, G, c_z = compose_xattn_pool(query, qn, mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias,
                                   le.weight, le.bias, 8)
    assert C.dtype == G.dtype == c_z.dtype == f8
    with torch.no_grad():
        want, u = _reference(h, 16, 2, query.double(), tuple(t.double() if torch.is_tensor(t) else t for t in qn), kvn,
                             mha.double(), le.double())
        a = torch.softmax((u @ G.T).reshape(16, 2, 8), dim=1)
        got = (a.unsqueeze(-1) * (u @ C.T).reshape(16, 2, 8, -1)).sum((1, 2)) + c_z
    assert _rel(got, want) <= 1e-12
