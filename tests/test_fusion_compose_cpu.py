"""CPU checks of the layer-0 fold of the fusion transformer (models.compose_qkv0): embed2latent -> norm1 -> in_proj equals the
composed short-K product with one factor per row, in fp64."""
import pytest
import torch

from madrigal_amd.models import compose_qkv0

f8 = torch.float64


def _params(D, d, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=f8)                     # noqa: E731
    We, be = r(d, D) / D ** 0.5, r(d)
    Wq, bq = r(3 * d, d) / d ** 0.5, r(3 * d)
    g1, b1 = 1.0 + 0.5 * r(d), r(d)                                          # non-trivial gamma / beta
    return We, be, Wq, bq, g1, b1


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("D,d", [(128, 512), (128, 2048)])
@pytest.mark.parametrize("offset", [0.0, 1e3])
def test_prenorm_fold_matches_ln_then_linear(D, d, offset):
    We, be, Wq, bq, g1, b1 = _params(D, d, 1)
    g = torch.Generator().manual_seed(2)
    T = torch.randn(300, D, generator=g, dtype=f8) + offset                  # tokens with a large common offset
    eps = 1e-5
    h = T @ We.T + be
    want = torch.nn.functional.layer_norm(h, (d,), g1, b1, eps) @ Wq.T + bq
    M, c, c2 = compose_qkv0(We, be, Wq, bq, (g1, b1))
    rstd = 1.0 / torch.sqrt(h.var(1, unbiased=False, keepdim=True) + eps)
    got = rstd * (T @ M.T + c) + c2
    assert M.shape == (3 * d, D) and c.shape == (3 * d,) and c2.shape == (3 * d,)
    assert _rel(got, want) <= 1e-12


@pytest.mark.parametrize("D,d", [(128, 512), (128, 2048)])
def test_postnorm_fold_matches_linear_of_linear(D, d):
    We, be, Wq, bq, _, _ = _params(D, d, 3)
    T = torch.randn(300, D, generator=torch.Generator().manual_seed(4), dtype=f8) + 50.0
    want = (T @ We.T + be) @ Wq.T + bq
    M, c, c2 = compose_qkv0(We, be, Wq, bq, None)
    assert c is None
    assert _rel(T @ M.T + c2, want) <= 1e-12


def test_fold_takes_fp32_parameters_in_fp64():
    """The shipped parameters are fp32: the composite is formed in fp64 all the same (no cancellation in the centring)."""
    We, be, Wq, bq, g1, b1 = (t.float() for t in _params(128, 512, 5))
    M, c, c2 = compose_qkv0(We, be, Wq, bq, (g1, b1))
    assert M.dtype == c.dtype == c2.dtype == f8
    # the composite of the fp32 parameters reproduces LN -> linear evaluated in fp64 on the same (fp32-valued) parameters
    T = torch.randn(64, 128, generator=torch.Generator().manual_seed(6), dtype=f8)
    h = T @ We.double().T + be.double()
    want = torch.nn.functional.layer_norm(h, (512,), g1.double(), b1.double(), 1e-5) @ Wq.double().T + bq.double()
    rstd = 1.0 / torch.sqrt(h.var(1, unbiased=False, keepdim=True) + 1e-5)
    assert _rel(rstd * (T @ M.T + c) + c2, want) <= 1e-12
