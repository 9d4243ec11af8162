"""models.compose_layer0_tokenspace in fp64 against the block it folds: norm1 -> in_proj -> masked per-head softmax attention ->
out_proj + residual on h = embed2latent(T).  Everything here is fp64 on the CPU, so the bound is rounding alone: 1e-12 of the
output scale."""
import math

import pytest
import torch

from madrigal_amd.models import compose_layer0_tokenspace

BOUND = 1e-12
F8 = torch.float64
EPS = 1e-5


def _params(D, d, H, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F8)
    sig = math.sqrt(30.0 / d)                         # q . k / sqrt(dh) then has a spread of a few tens: logit spreads > 50
    p = {"We": r(d, D) / math.sqrt(D), "be": 0.5 * r(d), "g1": 1.0 + 0.3 * r(d), "b1": 0.2 * r(d),
         "Wi": torch.cat([sig * r(2 * d, d), r(d, d) / math.sqrt(d)]), "bi": 0.3 * r(3 * d),
         "Wo": r(d, d) / math.sqrt(d), "bo": 0.3 * r(d)}
    return p


def _tokens(D, seed, offset=0.0, n=6, S=7):
    g = torch.Generator().manual_seed(seed)
    T = torch.randn(n, S, D, generator=g, dtype=F8) + offset         # a common offset on every token entry
    live = torch.rand(n, S, generator=g) < 0.7
    live[:, 0] = True
    live[2] = False
    live[2, 3] = True                                                # a drug with a single live token
    src = torch.zeros(S, S, dtype=torch.bool)                        # True = query row may not attend key column
    src[:2, -2:] = True
    return T, live, src


def _reference(p, T, live, src, H):
    """(h1 [n, S, d], largest logit spread over the allowed keys of a row): the uncomposed block, drug by drug."""
    n, S, _ = T.shape
    d = p["We"].shape[0]
    dh = d // H
    h = T @ p["We"].T + p["be"]
    mu = h.mean(-1, keepdim=True)
    a = (h - mu) / torch.sqrt(h.var(-1, unbiased=False, keepdim=True) + EPS) * p["g1"] + p["b1"]
    q, k, v = ((a @ p["Wi"][i * d:(i + 1) * d].T + p["bi"][i * d:(i + 1) * d]).view(n, S, H, dh).transpose(1, 2) for i in range(3))
    logits = q @ k.transpose(-1, -2) / math.sqrt(dh)                                     # [n, H, S, S]
    blocked = src.view(1, 1, S, S) | ~live.view(n, 1, 1, S)
    lm = logits.masked_fill(blocked, float("-inf"))
    spread = (lm.amax(-1) - logits.masked_fill(blocked, float("inf")).amin(-1))[live.view(n, 1, S).expand(n, H, S)].max()
    att = (torch.softmax(lm, -1) @ v).transpose(1, 2).reshape(n, S, d)
    return att @ p["Wo"].T + p["bo"] + h, float(spread)


def _tokenspace(p, T, live, src, H):
    """The same rows from the composites, step by step as the kernels take them (r from R_f, X, U, attention on X, one dense block)."""
    A, bp, a, C, co, Rf = compose_layer0_tokenspace(p["We"], p["be"], p["Wi"], p["bi"], p["Wo"], p["bo"], p["g1"], p["b1"], H)
    n, S, D = T.shape
    d = p["We"].shape[0]
    Dp = A.shape[0] // H
    assert Dp == (D + 4) // 4 * 4 and C.shape == (d, H * Dp + D) and Rf.shape == (D + 1, D + 1)
    t1 = torch.cat([T, torch.ones(n, S, 1, dtype=F8)], -1)
    r = 1.0 / torch.sqrt((t1 @ Rf.T).pow(2).sum(-1, keepdim=True) / d + EPS)             # [n, S, 1]
    X = torch.nn.functional.pad(r * t1, (0, Dp - D - 1))                                 # [n, S, Dp]
    U = (r * (T @ A.T + bp) + a).view(n, S, H, Dp).transpose(1, 2)                       # [n, H, S, Dp]
    logits = U @ X.unsqueeze(1).transpose(-1, -2)
    blocked = src.view(1, 1, S, S) | ~live.view(n, 1, 1, S)
    O = (torch.softmax(logits.masked_fill(blocked, float("-inf")), -1) @ X.unsqueeze(1)).transpose(1, 2).reshape(n, S, H * Dp)
    return torch.cat([O, T], -1) @ C.T + co, r.squeeze(-1), (A, bp, a, C)


@pytest.mark.parametrize("offset", [0.0, 1e3])
@pytest.mark.parametrize("H", [1, 2, 8])
@pytest.mark.parametrize("d", [32, 512])
@pytest.mark.parametrize("D", [8, 128])
def test_tokenspace_composites_match_the_block(D, d, H, offset):
    """Both token sets run every (D, d, H): rows around zero, whose logits spread by more than 50 over a row's keys, and rows with a
    common offset of 10^3.  (Not both at once: behind the offset the normalised rows of a drug differ by ~1e-3, so a spread of 50
    needs logits of ~5e4, and the block itself -- folded or not -- then answers a 1e-16 change of T with more than 1e-12.)"""
    p = _params(D, d, H, 100 * D + d + H)
    T, live, src = _tokens(D, D + H, offset)
    want, spread = _reference(p, T, live, src, H)
    got, _, (A, bp, a, C) = _tokenspace(p, T, live, src, H)
    assert offset or spread > 50.0, spread
    assert all(bool((t != 0).any()) for t in (bp, a))                                    # the bias terms are in play
    Dp = A.shape[0] // H
    pads = torch.arange(H * Dp).view(H, Dp)[:, D + 1:].flatten()
    assert not A[pads].any() and not bp[pads].any() and not a[pads].any() and not C[:, pads].any()      # zero rows at the pads
    w, g_ = want[live], got[live]
    assert torch.isfinite(g_).all()
    err = float((g_ - w).abs().max() / w.abs().max())
    print(f"D={D} d={d} H={H} offset={offset:g}: spread {spread:.1f}, rel err {err:.2e}")
    assert err <= BOUND


@pytest.mark.parametrize("d", [32, 512])
@pytest.mark.parametrize("D", [8, 128])
def test_triangular_factor_gives_the_centred_norm(D, d):
    """|R_f [T; 1]| = |W_c T + b_c| (so r is norm1's factor), also where d < D + 1 leaves R_f with zero rows."""
    p = _params(D, d, 1, 7 * D + d)
    T, live, src = _tokens(D, 3, 1e3)
    _, r, _ = _tokenspace(p, T, live, src, 1)
    h = T @ p["We"].T + p["be"]
    hc = h - h.mean(-1, keepdim=True)
    Rf = compose_layer0_tokenspace(p["We"], p["be"], p["Wi"], p["bi"], p["Wo"], p["bo"], p["g1"], p["b1"], 1)[5]
    t1 = torch.cat([T, torch.ones(*T.shape[:2], 1, dtype=F8)], -1)
    nrm = (t1 @ Rf.T).norm(dim=-1)
    assert float(((nrm - hc.norm(dim=-1)).abs() / hc.norm(dim=-1)).max()) <= BOUND
    want = 1.0 / torch.sqrt(h.var(-1, unbiased=False) + EPS)
    assert float(((r - want).abs() / want).max()) <= BOUND
    assert not Rf.tril(-1).any()
