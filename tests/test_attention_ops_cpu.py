"""The float64 attention references and the compact-layout restatement of attention_ref.py, checked without a GPU: pack_tiles against
TransformerFusion.live_token_plan, the formulas against torch's scaled_dot_product_attention, and the input conditions that
test_attention_ops_gpu.py relies on (asserted here so that the reference alone meets them)."""
import pytest
import torch
import torch.nn.functional as F

import attention_ref as R


def _make_masks():
    from madrigal_amd import data
    return data.make_masks


def _case(name):
    return R.mask_case(name, _make_masks())


# ------------------------------------------------------------------------------------ 1. pack_tiles against live_token_plan
@pytest.mark.parametrize("name", R.MASK_CASES)
def test_pack_tiles_matches_live_token_plan(name):
    from madrigal_amd import models as M
    live, src = _case(name)
    n, S = live.shape
    m = M.TransformerFusion(128, 2, 1, 2, 32, 64, 0.0, "gelu", True, True, "mean")
    plan = m.live_token_plan(~live, src)
    mine = R.pack_tiles(live, src)
    assert plan["n"] == mine["n"] and plan["S"] == mine["S"] and plan["R"] == mine["R"] and plan["n_tiles"] == mine["n_tiles"]
    for key in ("tile_start", "row_bits", "token_index", "row_start"):
        assert plan[key].dtype == mine[key].dtype, key
        assert torch.equal(plan[key], mine[key]), key


def test_scatter_and_gather_compact_are_inverse():
    live, src = _case("mixed_tiles")
    plan = R.pack_tiles(live, src)
    n, S = live.shape
    rows = R.rand((plan["R"], 6), 1)
    dense = R.scatter_compact(rows, plan["token_index"], n, S)
    assert torch.equal(R.gather_compact(dense.view(n, S, 6), plan["token_index"]), rows)
    assert torch.equal(R.gather_compact(dense, plan["token_index"]), rows)
    assert torch.equal(dense.view(n, S, 6)[~live], torch.zeros(int((~live).sum()), 6))
    w = torch.rand(n, 2, S, S, dtype=torch.float64)
    loc, own = R.tile_local(plan, w)
    back = R.tile_to_dense(plan, loc, fill=-1.0)
    both = live.view(n, 1, S, 1) & live.view(n, 1, 1, S)
    assert torch.equal(back[both.expand_as(w)], w[both.expand_as(w)]) and bool((back[~both.expand_as(w)] == -1.0).all())
    assert int(own.sum()) == int((live.sum(1) ** 2).sum())


# ------------------------------------------------------------------------------------ 2. the formulas against torch
@pytest.mark.parametrize("n,S,H,dh", [(3, 19, 4, 32), (2, 32, 1, 64), (4, 1, 2, 8), (2, 23, 3, 96)])
def test_self_attention_ref_matches_sdpa(n, S, H, dh):
    kpm, src = R.dense_masks(n, S)
    allowed = R.dense_allowed(n, S, kpm, src)
    qkv = [R.rand((n, S, H, dh), s).double() for s in (1, 2, 3)]
    g = R.rand((n, S, H, dh), 4).double()
    mine = [t.clone().requires_grad_(True) for t in qkv]
    out = R.self_attention_ref(*mine, allowed)
    out.backward(g)
    theirs = [t.clone().requires_grad_(True) for t in qkv]
    ref = F.scaled_dot_product_attention(*(t.transpose(1, 2) for t in theirs), attn_mask=allowed.unsqueeze(1)).transpose(1, 2)
    ref.backward(g)
    assert float((out - ref).detach().abs().max()) <= 1e-12
    for a, b in zip(mine, theirs):
        assert float((a.grad - b.grad).abs().max()) <= 1e-12


@pytest.mark.parametrize("n,Tk,H,dh", [(5, 4, 8, 64), (3, 32, 1, 64), (2, 1, 4, 32), (3, 7, 2, 100)])
def test_pool_ref_matches_sdpa(n, Tk, H, dh):
    q0, k0, v0 = R.rand((H, dh), 1).double(), R.rand((n, Tk, H, dh), 2).double(), R.rand((n, Tk, H, dh), 3).double()
    g = R.rand((n, H, dh), 4).double()
    mine = [t.clone().requires_grad_(True) for t in (q0, k0, v0)]
    out = R.pool_ref(*mine)
    out.backward(g)
    q, k, v = (t.clone().requires_grad_(True) for t in (q0, k0, v0))
    ref = F.scaled_dot_product_attention(q.view(1, H, 1, dh).expand(n, H, 1, dh), k.transpose(1, 2), v.transpose(1, 2))[:, :, 0]
    ref.backward(g)
    assert float((out - ref).detach().abs().max()) <= 1e-12
    for a, b in zip(mine, (q, k, v)):
        assert float((a.grad - b.grad).abs().max()) <= 1e-12


def test_dropout_factor_of_the_references():
    """keep / (1 - p) multiplies the weights after the softmax: all-ones keep scales the output, all-zeros keep gives zero."""
    n, S, H, dh = 2, 5, 2, 8
    q, k, v = (R.rand((n, S, H, dh), s).double() for s in (1, 2, 3))
    ok = R.dense_allowed(n, S)
    base = R.self_attention_ref(q, k, v, ok)
    assert float((R.self_attention_ref(q, k, v, ok, torch.ones(n, H, S, S), 0.5) - 2 * base).abs().max()) <= 1e-12
    assert float(R.self_attention_ref(q, k, v, ok, torch.zeros(n, H, S, S), 0.5).abs().max()) == 0.0
    keep = torch.zeros(n, H, S, S)
    keep[..., 1] = 1.0                                # only key 1 kept: the output is P[.., 1] v[1] / (1 - p)
    _, P = R.self_attention_ref(q, k, v, ok, want_probs=True)
    want = torch.einsum("nhi,nhd->nihd", P[..., 1], v[:, 1]) / 0.75
    assert float((R.self_attention_ref(q, k, v, ok, keep, 0.25) - want).abs().max()) <= 1e-12
    pq, pk, pv = R.rand((H, dh), 4).double(), R.rand((n, S, H, dh), 5).double(), R.rand((n, S, H, dh), 6).double()
    assert float((R.pool_ref(pq, pk, pv, torch.ones(n, H, S), 0.5) - 2 * R.pool_ref(pq, pk, pv)).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------ 3. input conditions of the GPU tests
@pytest.mark.parametrize("S,H,dh", R.DENSE_SHAPES + R.DROPOUT_DENSE_SHAPES)
def test_dense_cases_leave_every_query_a_key(S, H, dh):
    kpm, src = R.dense_masks(R.DENSE_N, S)
    assert bool(R.dense_allowed(R.DENSE_N, S, kpm, src).any(-1).all())
    assert bool(kpm.any()) or S == 1                                     # and the key padding is not empty


@pytest.mark.parametrize("name", R.MASK_CASES)
def test_compact_cases_hold_the_tiles_they_claim(name):
    live, src = _case(name)
    plan = R.pack_tiles(live, src)
    n, S = live.shape
    rows = (plan["tile_start"][1:] - plan["tile_start"][:-1]).tolist()
    counts = live.sum(1).tolist()
    assert sum(rows) == plan["R"] == int(live.sum()) and max(rows) <= 32 and min(rows) >= 1
    drugs_per_tile = [len(set(plan["row_drug"][plan["row_tile"] == t].tolist())) for t in range(plan["n_tiles"])]
    allowed = R.compact_allowed(live, src)
    assert bool(allowed[live].any(-1).all())                             # every live query row has a key
    if name == "mixed_tiles":
        assert S == 21 and src is None
        assert rows == [sum(R.MIXED_SMALL), 32, 1] and drugs_per_tile == [10, 2, 1]
        assert counts == R.MIXED_SMALL + [19, 13, 1] and all(1 <= c <= 3 for c in R.MIXED_SMALL)
    elif name == "source_mask":
        assert S == 21 and src is not None and bool(src[:3, -16:].all()) and bool(src[-16:, :3].all()) and int(src.sum()) == 96
        assert bool(live[:, 3:5].all()) and max(drugs_per_tile) >= 2 and plan["n_tiles"] >= 2
        assert bool((live.unsqueeze(1) & live.unsqueeze(2) & src.unsqueeze(0)).any())      # the source mask blocks live pairs
    elif name == "full_drugs":
        assert S == 32 and src is None and rows == [32, 32, 32] and drugs_per_tile == [1, 1, 1]
    else:
        assert (n, S) == (37, 24) and src is not None and not bool(src[0].any()) and not bool(src[:, 0].any())
        assert plan["n_tiles"] >= 4 and max(drugs_per_tile) >= 3 and len(set(counts)) >= 4


def test_dropout_cases_keep_every_allowed_weight_above_the_floor():
    """Mask recovery reads an entry as dropped when it is an exact 0 and as kept when it is within the tolerance of P / (1 - p):
    with every allowed weight >= 1e-3 and a tolerance of at most 4e-5 the two readings cannot both fit."""
    mm = _make_masks()
    for S, H, dh in R.DROPOUT_DENSE_SHAPES:
        kpm, src = R.dense_masks(R.DENSE_N, S)
        allowed = R.dense_allowed(R.DENSE_N, S, kpm, src)
        qkv, dout = R.dense_inputs(S, H, dh, scale=R.DROPOUT_QK_SCALE)
        _, _, P = R.attention_rows_ref(qkv, dout, R.DENSE_N, S, H, dh, allowed)
        ok = allowed.unsqueeze(1).expand_as(P)
        assert float(P[ok].min()) >= R.MIN_WEIGHT and float(P[~ok].abs().max()) == 0.0
    plan, _, _, allowed, _, _, P = R.compact_reference("mixed_tiles", 4, 32, mm, R.DROPOUT_QK_SCALE)
    loc, own = R.tile_local(plan, P)
    assert float(loc[own.unsqueeze(1).expand_as(loc)].min()) >= R.MIN_WEIGHT
    for Tk, H, dh in R.POOL_SHAPES:
        assert Tk <= dh
        q, kv, dout = R.pool_inputs(R.DROPOUT_POOL_N, Tk, H, dh, scale=R.DROPOUT_QK_SCALE)
        P = R.pool_rows_ref(q, kv, dout, R.DROPOUT_POOL_N, Tk, H, dh)[3]
        assert float(P.min()) >= R.MIN_WEIGHT
    for p in R.DROPOUT_P:
        assert R.TOL * max(1.0 / (1.0 - p), 1.0) < R.MIN_WEIGHT / 2


def test_fully_masked_drug_in_the_reference():
    """Group E's input: drug 1 has every key padded.  Autograd of the plain formula gives NaN value gradients there and keeps the
    other drugs finite."""
    n, S, H, dh = 3, 19, 2, 32
    kpm, src = R.dense_masks(n, S)
    kpm[1, :] = True
    allowed = R.dense_allowed(n, S, kpm, src)
    assert not bool(allowed[1].any()) and bool(allowed[0].any(-1).all()) and bool(allowed[2].any(-1).all())
    qkv, dout = R.dense_inputs(S, H, dh, n=n)
    out, dqkv, _ = R.attention_rows_ref(qkv, dout, n, S, H, dh, allowed)
    out, dqkv = out.view(n, S, -1), dqkv.view(n, S, -1)
    assert bool(torch.isnan(out[1]).all()) and bool(torch.isnan(dqkv[1, :, 2 * H * dh:]).all())
    assert bool(torch.isfinite(out[[0, 2]]).all()) and bool(torch.isfinite(dqkv[[0, 2]]).all())
