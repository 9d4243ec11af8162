"""Checkpoint-ensemble spread on the GPU: ops.bilinear_ensemble_spread (mean / std / bound, dense), ops.bilinear_ensemble_spread_topk
(top-k by the bound, each entry with its mean and std), pipeline.ensemble_spread_all_pairs / ensemble_confident_partners.

What is compared with what (L = 2, D = 128 throughout; inputs as test_ensemble_topk_gpu.py's: z ~ N(0,1) * scale, W ~ N(0,1) /
sqrt(128), symmetrised; scale 0.3 is unsaturated, at scale 1.0 many probabilities are exactly 1):
  mean   ``torch.equal`` to the general sweep of ops.bilinear_ensemble_sigmoid (cloned tails, so the mirrored sweep is not chosen).
  std    against float64 of the K single-model tensors of the existing product: |std - spread64| <= 2 e_p + 2 E_R.  e_p is measured
         on existing code alone -- the largest difference between the float64 mean of those K tensors and the existing K-model
         tensor; std is 1-Lipschitz in each p_m, so an error of e_p per model moves it by at most e_p.  E_R is the recurrence's own
         error (spread_ref.E_R, measured without a GPU); the factors 2 are the margin for the square root's rounding near zero.
         Observed (MI355X, the shapes below, K = 1..8, both scales): largest e_p 1.36e-07 (bf16x3) / 1.31e-07 (f32), largest
         |std - spread64| 8.35e-08 / 8.01e-08 (the test prints every case's figures).
  bound  one rounding of kappa * std + mean; kappa = 0 gives the mean bit for bit; a second call and a pitched ``out`` agree.
  top-k  exactly the stable sort of the dense bound of the same feature, mean and std gathered at idx; with kappa = 0 exactly
         ops.bilinear_ensemble_topk.  Every comparison of lists is ``torch.equal``."""
import functools

import numpy as np
import pytest
import torch

import spread_ref as R

pytestmark = pytest.mark.gpu

NEG = float("-inf")
SHAPES = ["1x1", "33x65", "129x130", "chunk-1", "chunk", "chunk+1", "300x1001"]


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _shape(name):
    from madrigal_amd import ops
    chunk = 64 * ops.bilinear_ensemble_spread_chunk_tiles()
    return {"1x1": (1, 1), "33x65": (33, 65), "129x130": (129, 130), "chunk-1": (129, chunk - 1), "chunk": (129, chunk),
            "chunk+1": (129, chunk + 1), "300x1001": (300, 1001)}[name]


@functools.lru_cache(maxsize=None)
def _inputs(K, nh, nt, L, scale, same, seed=0):
    """(zh, zt, ws) on the card.  Shared; never modified."""
    from madrigal_amd import ops
    zh = [_rand((nh, 128), 1000 * seed + 10 * m, scale).cuda() for m in range(K)]
    zt = zh if same else [_rand((nt, 128), 1000 * seed + 10 * m + 1, scale).cuda() for m in range(K)]
    ws = [ops.symmetrize(_rand((L, 128, 128), 1000 * seed + 10 * m + 2, 1 / np.sqrt(128)).cuda()) for m in range(K)]
    return zh, zt, ws


def _sigmoid_general(zh, zt, ws, prec):
    """The existing dense product, general sweep (the clone on the tail side keeps the mirrored sweep away)."""
    from madrigal_amd import ops
    return ops.bilinear_ensemble_sigmoid(zh, [t.clone() for t in zt], ws, precision=prec).contiguous()


@functools.lru_cache(maxsize=None)
def _dense(K, nh, nt, scale, prec, same, kappa=None):
    """The feature's own dense product, contiguous: (mean, std) or (mean, std, bound).  Shared; never modified."""
    from madrigal_amd import ops
    zh, zt, ws = _inputs(K, nh, nt, 2, scale, same)
    return tuple(t.contiguous() for t in ops.bilinear_ensemble_spread(zh, zt, ws, kappa=kappa, precision=prec))


def _allowed(nh, nt, eligible, device="cuda"):
    i = torch.arange(nh, device=device)[:, None]
    j = torch.arange(nt, device=device)[None, :]
    if eligible == "all":
        return torch.ones((nh, nt), dtype=torch.bool, device=device)
    return (j != i) if eligible == "not_self" else (j < i)


def _expected(dense, k, eligible, excluded=None):
    """(bound, idx, mean, std) [L,nh,k] of the dense (mean, std, bound) under the order (bound descending, column ascending):
    ineligible and excluded bounds -inf, a stable descending sort truncated to k, pads -inf / -1 / NaN / NaN."""
    mean, std, bound = dense
    L, nh, nt = bound.shape
    Q = torch.where(_allowed(nh, nt, eligible, bound.device)[None], bound, torch.full_like(bound, NEG))
    if excluded is not None:
        Q = Q.masked_fill(excluded.expand(L, nh, nt), NEG)
    v, i = torch.sort(Q, dim=2, descending=True, stable=True)
    v, i = v[:, :, :k], i[:, :, :k]
    if nt < k:
        v = torch.cat([v, torch.full((L, nh, k - nt), NEG, device=bound.device)], 2)
        i = torch.cat([i, torch.zeros((L, nh, k - nt), dtype=i.dtype, device=bound.device)], 2)
    dead = v == NEG
    nan = torch.full_like(v, float("nan"))
    m = torch.where(dead, nan, mean.gather(2, i))
    s = torch.where(dead, nan, std.gather(2, i))
    return v, torch.where(dead, torch.full_like(i, -1), i).to(torch.int32), m, s


def _same(a, b):
    """torch.equal that takes NaN pads as equal to NaN pads."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and \
        torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


def _check(got, want):
    assert [t.dtype for t in got] == [torch.float32, torch.int32, torch.float32, torch.float32]
    for g, w, name in zip(got, want, ("bound", "idx", "mean", "std")):
        assert _same(g, w), f"{name} differs"
    pad = got[1] == -1
    assert torch.equal(pad, got[0] == NEG) and torch.equal(pad, torch.isnan(got[2])) and torch.equal(pad, torch.isnan(got[3]))


# ---- 1. mean ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("scale", [0.3, 1.0])
@pytest.mark.parametrize("K", [1, 2, 5, 8])
@pytest.mark.parametrize("shape", SHAPES)
def test_mean_is_the_existing_dense_product_bit_for_bit(shape, K, scale, prec):
    nh, nt = _shape(shape)
    zh, zt, ws = _inputs(K, nh, nt, 2, scale, False)
    mean, std = _dense(K, nh, nt, scale, prec, False)
    assert mean.shape == std.shape == (2, nh, nt)
    assert torch.equal(mean, _sigmoid_general(zh, zt, ws, prec))


# ---- 2. std against float64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("scale", [0.3, 1.0])
@pytest.mark.parametrize("K", [1, 2, 5, 8])
@pytest.mark.parametrize("shape", ["33x65", "chunk+1", "300x1001"])
def test_std_against_float64_of_the_single_model_tensors(shape, K, scale, prec):
    nh, nt = _shape(shape)
    zh, zt, ws = _inputs(K, nh, nt, 2, scale, False)
    per_model = np.stack([_sigmoid_general(zh[m:m + 1], zt[m:m + 1], ws[m:m + 1], prec).cpu().numpy() for m in range(K)])
    mean64, std64 = R.spread64(per_model)
    e_p = float(np.abs(mean64 - _sigmoid_general(zh, zt, ws, prec).cpu().numpy().astype(np.float64)).max())     # existing code only
    std = _dense(K, nh, nt, scale, prec, False)[1]
    err = float(np.abs(std.cpu().numpy().astype(np.float64) - std64).max())
    print(f"{shape} K={K} scale={scale} {prec}: e_p {e_p:.3e}, |std - spread64| {err:.3e}, largest std {float(std64.max()):.3e}")
    assert err <= 2 * e_p + 2 * R.E_R
    assert bool((std >= 0).all()) and not bool(torch.isnan(std).any())
    if K == 1:
        assert not bool(std.any())
    else:
        assert float(std.max()) > 1e-3                    # the models do disagree: the comparison is not of zeros


# ---- 3. one checkpoint K times ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("scale", [0.3, 1.0])
def test_one_checkpoint_passed_five_times_has_no_spread(scale, prec):
    from madrigal_amd import ops
    zh, zt, ws = _inputs(1, 129, 130, 2, scale, False)
    five = lambda ts: [ts[0].clone() for _ in range(5)]   # noqa: E731
    mean, std, bound = ops.bilinear_ensemble_spread(five(zh), five(zt), five(ws), kappa=-1.0, precision=prec)
    assert not bool(std.any()) and not bool(torch.signbit(std).any())
    assert torch.equal(bound, mean)
    got = ops.bilinear_ensemble_spread_topk(five(zh), five(zt), five(ws), 16, -1.0, precision=prec)
    assert not bool(got[3].any()) and torch.equal(got[0], got[2])


# ---- 4. bound --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("K,scale", [(5, 0.3), (2, 1.0), (8, 1.0)])
@pytest.mark.parametrize("kappa", [-1.0, 0.5, 0.0, 0.3])     # 0.3: the one kappa here whose product with std is not exact in fp32
def test_bound_is_one_rounding_and_agrees_between_calls_and_layouts(kappa, K, scale, prec):
    from madrigal_amd import ops
    nh, nt = 129, 130
    zh, zt, ws = _inputs(K, nh, nt, 2, scale, False)
    mean, std, bound = _dense(K, nh, nt, scale, prec, False, kappa)
    plain = _dense(K, nh, nt, scale, prec, False)
    assert torch.equal(mean, plain[0]) and torch.equal(std, plain[1])
    if kappa == 0.0:
        assert torch.equal(bound, mean)
    # one rounding: within half an ulp of the exact kappa * std + mean (the product is exact in float64)
    exact = float(np.float32(kappa)) * std.double() + mean.double()
    half_ulp = torch.exp2((torch.frexp(exact).exponent - 25).double())
    assert bool(((bound.double() - exact).abs() <= half_ulp * (1 + 1e-6)).all())
    # a second call that writes the bound alone
    alone = torch.full((2, nh, nt), float("nan"), device="cuda")
    back = ops.bilinear_ensemble_spread(zh, zt, ws, kappa=kappa, precision=prec, out=(None, None, alone))
    assert back[0] is None and back[1] is None and back[2] is alone and torch.equal(alone, bound)
    # row-pitched views with one pitch: every entry written, nothing beside them
    store = [torch.full((2, nh, nt + 7), -5.0, device="cuda") for _ in range(3)]
    views = tuple(s[:, :, :nt] for s in store)
    back = ops.bilinear_ensemble_spread(zh, zt, ws, kappa=kappa, precision=prec, out=views)
    assert all(b is v for b, v in zip(back, views))
    for s, want in zip(store, (mean, std, bound)):
        assert torch.equal(s[:, :, :nt], want) and bool((s[:, :, nt:] == -5.0).all())
    with pytest.raises(ValueError, match="one row pitch"):
        ops.bilinear_ensemble_spread(zh, zt, ws, kappa=kappa, precision=prec, out=(views[0], torch.empty((2, nh, nt), device="cuda"), views[2]))


# ---- 5. top-k against the dense product of the same feature ---------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("scale", [0.3, 1.0])
@pytest.mark.parametrize("K", [2, 5, 8])
@pytest.mark.parametrize("shape", SHAPES)
def test_topk_is_the_sorted_dense_bound_with_its_mean_and_std(shape, K, scale, prec):
    from madrigal_amd import ops
    nh, nt = _shape(shape)
    zh, zt, ws = _inputs(K, nh, nt, 2, scale, False)
    kappa = -1.0 if K != 5 else 0.5
    dense = _dense(K, nh, nt, scale, prec, False, kappa)
    for k in (1, 16, 32):
        _check(ops.bilinear_ensemble_spread_topk(zh, zt, ws, k, kappa, precision=prec), _expected(dense, k, "all"))


def test_the_bound_reorders_the_means_list():
    """kappa = -1 is not a relabelling of the mean's ranking: among a row's 16 best the two lists differ in most rows."""
    from madrigal_amd import ops
    zh, zt, ws = _inputs(5, 300, 1001, 2, 0.3, False)
    by_bound = ops.bilinear_ensemble_spread_topk(zh, zt, ws, 16, -1.0)[1]
    by_mean = ops.bilinear_ensemble_topk(zh, zt, ws, 16)[1]
    assert float((by_bound != by_mean).any(dim=2).float().mean()) > 0.5


# ---- 6. top-k against existing code ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("K,scale", [(5, 0.3), (1, 1.0), (2, 1.0)])
@pytest.mark.parametrize("eligible", ["all", "not_self", "lower"])
@pytest.mark.parametrize("N", [1, 2, 129, 300])
def test_kappa_zero_is_the_existing_topk(N, eligible, K, scale, prec):
    from madrigal_amd import ops
    z, _, ws = _inputs(K, N, N, 2, scale, True)
    for k in (1, 16, 32):
        got = ops.bilinear_ensemble_spread_topk(z, z, ws, k, 0.0, eligible=eligible, precision=prec)
        vals, idx = ops.bilinear_ensemble_topk(z, z, ws, k, eligible=eligible, precision=prec)
        assert torch.equal(got[0], vals) and torch.equal(got[1], idx)
        assert _same(got[2], torch.where(idx < 0, torch.full_like(vals, float("nan")), vals))     # the mean is the bound here


# ---- 7. masks, duplicates, determinism -------------------------------------------------------------------------------------------
def _random_pairs(N, frac, seed):
    g = torch.Generator().manual_seed(seed)
    n = int(N * N * frac)
    return torch.randint(0, N, (n,), generator=g), torch.randint(0, N, (n,), generator=g)


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("K,scale", [(5, 0.3), (2, 1.0)])
@pytest.mark.parametrize("planes", ["shared", "per_outcome"])
@pytest.mark.parametrize("eligible", ["not_self", "lower", "all"])
def test_exclusion_masks(eligible, planes, K, scale, prec):
    from madrigal_amd import ops
    N, L, k, kappa = 300, 2, 32, -1.0
    z, _, ws = _inputs(K, N, N, L, scale, True)
    dense = _dense(K, N, N, scale, prec, True, kappa)
    h, t = _random_pairs(N, 0.01, 5)                                       # 1 % of the pairs
    best40 = _expected(dense, 32, eligible)[1][0, 200].cpu().long()        # outcome 0, row 200: its best eligible columns
    best40 = best40[best40 >= 0]
    h = torch.cat([h, torch.full((N,), 7), torch.full((best40.numel(),), 200)])        # row 7 entirely, row 200's best
    t = torch.cat([t, torch.arange(N), best40])
    sym = eligible == "not_self"
    if planes == "shared":
        mask = ops.pair_mask(h, t, N, symmetric=sym, device="cuda")
    else:
        lab = torch.cat([torch.arange(h.numel() - best40.numel()) % L, torch.zeros(best40.numel(), dtype=torch.int64)])
        mask = ops.pair_mask(h, t, N, labels=lab, n_labels=L, symmetric=sym, device="cuda")
    excluded = ops.pair_mask_dense(mask, N, N)
    got = ops.bilinear_ensemble_spread_topk(z, z, ws, k, kappa, eligible=eligible, precision=prec, exclude=mask)
    _check(got, _expected(dense, k, eligible, excluded))
    if planes == "shared":
        assert bool((got[1][:, 7] == -1).all())                            # a fully excluded row is all padding
    assert not bool(torch.isin(got[1][0, 200].cpu().long(), best40).any())


@pytest.mark.parametrize("eligible", ["all", "lower"])
def test_no_mask_and_an_all_zero_mask_agree(eligible):
    from madrigal_amd import ops
    z, _, ws = _inputs(5, 300, 300, 2, 0.3, True)
    none = ops.bilinear_ensemble_spread_topk(z, z, ws, 16, -1.0, eligible=eligible)
    for P in (1, 2):
        zero = torch.zeros((P, (300 + 31) // 32, 320), dtype=torch.int32, device="cuda")
        _check(ops.bilinear_ensemble_spread_topk(z, z, ws, 16, -1.0, eligible=eligible, exclude=zero), none)


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("K,scale", [(5, 0.3), (2, 1.0)])
def test_duplicated_tail_rows_keep_both_copies_in_column_order(K, scale, prec):
    """Tail rows j and j + 193 are the same drug: equal bounds in different lanes, tiles and chunks."""
    from madrigal_amd import ops
    zh = [_rand((130, 128), 70 + m, scale).cuda() for m in range(K)]
    half = [_rand((193, 128), 80 + m, scale).cuda() for m in range(K)]
    zt = [torch.cat([a, a]).contiguous() for a in half]
    ws = [ops.symmetrize(_rand((2, 128, 128), 90 + m, 1 / np.sqrt(128)).cuda()) for m in range(K)]
    dense = tuple(t.contiguous() for t in ops.bilinear_ensemble_spread(zh, zt, ws, kappa=-1.0, precision=prec))
    assert all(torch.equal(t[:, :, :193], t[:, :, 193:]) for t in dense)
    got = ops.bilinear_ensemble_spread_topk(zh, zt, ws, 32, -1.0, precision=prec)
    _check(got, _expected(dense, 32, "all"))
    if scale == 0.3:                                   # distinct bounds: the list is 16 pairs (j, j + 193), the smaller column first
        assert torch.equal(got[1][:, :, 0::2] + 193, got[1][:, :, 1::2])
        for t in (got[0], got[2], got[3]):
            assert torch.equal(t[:, :, 0::2], t[:, :, 1::2])


@pytest.mark.parametrize("K,scale", [(5, 0.3), (2, 1.0)])
def test_two_calls_agree_and_out_is_filled(K, scale):
    from madrigal_amd import ops
    zh, zt, ws = _inputs(K, 300, 1001, 2, scale, False)
    a = ops.bilinear_ensemble_spread_topk(zh, zt, ws, 32, -1.0)
    _check(ops.bilinear_ensemble_spread_topk(zh, zt, ws, 32, -1.0), a)
    f = lambda v: torch.full((2, 300, 32), v, device="cuda")              # noqa: E731
    out = (f(3.0), torch.full((2, 300, 32), -7, dtype=torch.int32, device="cuda"), f(3.0), f(3.0))
    back = ops.bilinear_ensemble_spread_topk(zh, zt, ws, 32, -1.0, out=out)
    assert all(b is o for b, o in zip(back, out))
    _check(out, a)
    d1 = ops.bilinear_ensemble_spread(zh, zt, ws, kappa=-1.0)
    d2 = ops.bilinear_ensemble_spread(zh, zt, ws, kappa=-1.0)
    assert all(torch.equal(x, y) for x, y in zip(d1, d2))
    with pytest.raises(ValueError):
        ops.bilinear_ensemble_spread_topk(zh, zt, ws, 32, -1.0, out=(out[0][:, :, :16], out[1], out[2], out[3]))
    with pytest.raises(ValueError, match="one drug set"):
        ops.bilinear_ensemble_spread_topk(zh, zt, ws, 4, -1.0, eligible="not_self")


# ---- 8. pipeline -----------------------------------------------------------------------------------------------------------------
def test_the_pipeline_functions_on_a_model_pair():
    """Two checkpoints' original head weights, 300 drugs, 4 outcomes: ensemble_confident_partners with drug_rows, label_range and
    exclude is ensemble_spread_all_pairs sorted; with kappa = 0 it is ensemble_top_partners."""
    from madrigal_amd import models as M, ops
    from madrigal_amd.pipeline import ensemble_confident_partners, ensemble_spread_all_pairs, ensemble_top_partners
    K, N, L = 2, 300, 4
    w = [_rand((L, 128, 128), 40 + m, 1 / np.sqrt(128)).cuda() for m in range(K)]
    zs = [_rand((N, 128), 50 + m, 0.3).cuda() for m in range(K)]
    h, t = _random_pairs(N, 0.01, 9)
    known = ops.pair_mask(h, t, N, symmetric=True, device="cuda")
    with M.precision("bf16x3"):
        dense = tuple(x.contiguous() for x in ensemble_spread_all_pairs(w, zs, kappa=-1.0))
        assert len(ensemble_spread_all_pairs(w, zs, label_range=(1, 3))) == 2
        assert torch.equal(ensemble_spread_all_pairs(w, zs, label_range=(1, 3))[1], dense[1][1:3])
        full = ensemble_confident_partners(w, zs, 8)
        _check(full, _expected(dense, 8, "not_self"))
        rows = [299, 3, 150, 3, 0, 77]
        part = ensemble_confident_partners(w, zs, 8, kappa=-1.0, label_range=(1, 4), drug_rows=rows, exclude=known)
        want = _expected(tuple(x[1:4] for x in dense), 8, "not_self", ops.pair_mask_dense(known, N, N))
        _check(part, tuple(x[:, rows] for x in want))
        lower = ensemble_confident_partners(w, zs, 8, kappa=0.5, eligible="lower")
        _check(lower, _expected(tuple(x.contiguous() for x in ensemble_spread_all_pairs(w, zs, kappa=0.5)), 8, "lower"))
        zero = ensemble_confident_partners(w, zs, 8, kappa=0.0, label_range=(1, 4), drug_rows=rows, exclude=known)
        vals, idx = ensemble_top_partners(w, zs, 8, label_range=(1, 4), drug_rows=rows, exclude=known)
        assert torch.equal(zero[0], vals) and torch.equal(zero[1], idx)
