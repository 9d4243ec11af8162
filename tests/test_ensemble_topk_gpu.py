"""Top-k screening over a checkpoint ensemble on the GPU (ops.bilinear_ensemble_topk, pipeline.ensemble_top_partners /
ensemble_top_pairs) against the dense ensemble product, exactly.

The reference is always the GENERAL ensemble sweep on the card: ``ops.bilinear_ensemble_sigmoid(zh, [t.clone() for t in zt], ws)`` (the
clone on the tail side forces the non-mirrored sweep, whose values (z_i W) z_j are the ones the lists see), ineligible and excluded
entries set to -inf, a stable descending sort (= value descending, column ascending) truncated to k, index -1 where the value is
-inf.  Every comparison is ``torch.equal`` on values and on indices: no tolerance is involved.

Two input regimes (z ~ N(0,1) * scale, W ~ N(0,1) / sqrt(128), symmetrised):
  scale 0.3: no probability equals 1 and a row's 32 best have no equal neighbours -- tests the values;
  scale 1.0: several per cent of all probabilities are exactly 1.0 at K = 1 and nearly all neighbours among a row's 32 best are
             equal -- tests the tie rule across lanes, tiles and chunks with no special construction."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NEG = float("-inf")


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


@functools.lru_cache(maxsize=None)
def _case(K, nh, nt, L, scale, prec, same, seed=0):
    """Inputs on the card and their dense general-sweep product: (zh, zt, ws, P [L,nh,nt] contiguous).  Shared; never modified."""
    from madrigal_amd import ops
    zh = [_rand((nh, 128), 1000 * seed + 10 * m, scale).cuda() for m in range(K)]
    zt = zh if same else [_rand((nt, 128), 1000 * seed + 10 * m + 1, scale).cuda() for m in range(K)]
    ws = [ops.symmetrize(_rand((L, 128, 128), 1000 * seed + 10 * m + 2, 1 / np.sqrt(128)).cuda()) for m in range(K)]
    return zh, zt, ws, _dense(zh, zt, ws, prec)


def _dense(zh, zt, ws, prec):
    from madrigal_amd import ops
    return ops.bilinear_ensemble_sigmoid(zh, [t.clone() for t in zt], ws, precision=prec).contiguous()


def _allowed(nh, nt, eligible, device="cuda"):
    i = torch.arange(nh, device=device)[:, None]
    j = torch.arange(nt, device=device)[None, :]
    if eligible == "all":
        return torch.ones((nh, nt), dtype=torch.bool, device=device)
    return (j != i) if eligible == "not_self" else (j < i)


def _expected(P, k, eligible, excluded=None):
    """(vals [L,nh,k], idx [L,nh,k] int32) of the dense P under the order (value descending, column ascending)."""
    L, nh, nt = P.shape
    Q = torch.where(_allowed(nh, nt, eligible, P.device)[None], P, torch.full_like(P, NEG))
    if excluded is not None:
        Q = Q.masked_fill(excluded.expand(L, nh, nt), NEG)
    v, i = torch.sort(Q, dim=2, descending=True, stable=True)
    v, i = v[:, :, :k], i[:, :, :k].to(torch.int32)
    if nt < k:
        v = torch.cat([v, torch.full((L, nh, k - nt), NEG, device=P.device)], 2)
        i = torch.cat([i, torch.full((L, nh, k - nt), -1, dtype=torch.int32, device=P.device)], 2)
    return v, torch.where(v == NEG, torch.full_like(i, -1), i)


def _check(got, want):
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32
    assert torch.equal(got[0], want[0]), "values differ"
    assert torch.equal(got[1], want[1]), "indices differ"


def _shape(name):
    from madrigal_amd import ops
    chunk = 64 * ops.bilinear_ensemble_topk_chunk_tiles()
    return {"1x1": (1, 1), "33x65": (33, 65), "129x130": (129, 130), "chunk-1": (129, chunk - 1), "chunk": (129, chunk),
            "chunk+1": (129, chunk + 1), "300x1001": (300, 1001)}[name]


# ---- sizes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("scale", [0.3, 1.0])
@pytest.mark.parametrize("K", [1, 2, 5, 8])
@pytest.mark.parametrize("shape", ["1x1", "33x65", "129x130", "chunk-1", "chunk", "chunk+1", "300x1001"])
def test_sizes_against_the_dense_product(shape, K, scale, prec):
    from madrigal_amd import ops
    nh, nt = _shape(shape)
    zh, zt, ws, P = _case(K, nh, nt, 2, scale, prec, False)
    for k in (1, 16, 32):
        _check(ops.bilinear_ensemble_topk(zh, zt, ws, k, precision=prec), _expected(P, k, "all"))


def test_the_two_regimes_are_what_the_docstring_says():
    """Scale 1.0, K = 1: exact ones and ties among the best are the rule; scale 0.3, K = 5: neither occurs."""
    P1 = _case(1, 300, 1001, 2, 1.0, "bf16x3", False)[3]
    assert float((P1 == 1.0).float().mean()) > 0.01
    top = torch.sort(P1, dim=2, descending=True).values[:, :, :32]
    assert float((top[:, :, 1:] == top[:, :, :-1]).float().mean()) > 0.9
    P5 = _case(5, 300, 1001, 2, 0.3, "bf16x3", False)[3]
    assert not bool((P5 == 1.0).any())
    top = torch.sort(P5, dim=2, descending=True).values[:, :, :32]
    assert float((top[:, :, 1:] == top[:, :, :-1]).float().mean()) < 0.01


# ---- eligibility ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("K,scale", [(5, 0.3), (1, 1.0), (2, 1.0)])
@pytest.mark.parametrize("eligible", ["not_self", "lower"])
@pytest.mark.parametrize("N", [1, 2, 129, 300])
def test_one_drug_set_against_itself(N, eligible, K, scale, prec):
    from madrigal_amd import ops
    z, _, ws, P = _case(K, N, N, 2, scale, prec, True)
    for k in (1, 16, 32):
        got = ops.bilinear_ensemble_topk(z, z, ws, k, eligible=eligible, precision=prec)
        _check(got, _expected(P, k, eligible))
        if eligible == "lower":                       # row 0 has no eligible column, row 5 has five
            assert bool((got[1][:, 0] == -1).all()) and bool((got[0][:, 0] == NEG).all())
            if N > 5:
                assert bool((got[1][:, 5, :min(k, 5)] >= 0).all()) and bool((got[1][:, 5, 5:] == -1).all())


@pytest.mark.parametrize("eligible", ["all", "not_self", "lower"])
def test_k_above_the_number_of_columns_pads(eligible):
    from madrigal_amd import ops
    z, _, ws, P = _case(5, 20, 20, 2, 0.3, "bf16x3", True)
    got = ops.bilinear_ensemble_topk(z, z, ws, 32, eligible=eligible)
    _check(got, _expected(P, 32, eligible))
    assert bool((got[1][:, :, 20:] == -1).all())


# ---- duplicates ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("K,scale", [(5, 0.3), (1, 1.0)])
def test_duplicated_tail_rows_keep_both_copies_in_column_order(K, scale, prec):
    """Tail rows j and j + 193 are the same drug: equal values in different lanes and tiles (for some j in different chunks)."""
    from madrigal_amd import ops
    zh = [_rand((130, 128), 70 + m, scale).cuda() for m in range(K)]
    half = [_rand((193, 128), 80 + m, scale).cuda() for m in range(K)]
    zt = [torch.cat([a, a]).contiguous() for a in half]
    ws = [ops.symmetrize(_rand((2, 128, 128), 90 + m, 1 / np.sqrt(128)).cuda()) for m in range(K)]
    P = _dense(zh, zt, ws, prec)
    assert torch.equal(P[:, :, :193], P[:, :, 193:])
    v, i = ops.bilinear_ensemble_topk(zh, zt, ws, 32, precision=prec)
    _check((v, i), _expected(P, 32, "all"))
    if scale == 0.3:                                   # distinct values: the list is 16 pairs (j, j + 193), the smaller column first
        assert torch.equal(i[:, :, 0::2] + 193, i[:, :, 1::2]) and torch.equal(v[:, :, 0::2], v[:, :, 1::2])


# ---- masks ---------------------------------------------------------------------------------------------------------------------
def _random_pairs(N, frac, seed):
    g = torch.Generator().manual_seed(seed)
    n = int(N * N * frac)
    return torch.randint(0, N, (n,), generator=g), torch.randint(0, N, (n,), generator=g)


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("K,scale", [(5, 0.3), (1, 1.0)])
@pytest.mark.parametrize("planes", ["shared", "per_outcome"])
@pytest.mark.parametrize("eligible", ["not_self", "lower", "all"])
def test_exclusion_masks(eligible, planes, K, scale, prec):
    from madrigal_amd import ops
    N, L, k = 300, 2, 32
    z, _, ws, P = _case(K, N, N, L, scale, prec, True)
    h, t = _random_pairs(N, 0.01, 5)                                       # 1 % of the pairs
    order = torch.sort(torch.where(_allowed(N, N, eligible)[None], P, torch.full_like(P, NEG)), dim=2, descending=True, stable=True).indices
    best40 = order[0, 200, :40].cpu()                                      # outcome 0, row 200: its 40 best eligible columns
    h = torch.cat([h, torch.full((N,), 7), torch.full((40,), 200)])        # row 7 entirely, row 200's 40 best
    t = torch.cat([t, torch.arange(N), best40])
    sym = eligible == "not_self"
    if planes == "shared":
        mask = ops.pair_mask(h, t, N, symmetric=sym, device="cuda")
    else:
        lab = torch.cat([torch.arange(h.numel() - 40) % L, torch.zeros(40, dtype=torch.int64)])     # row 200's columns under outcome 0
        mask = ops.pair_mask(h, t, N, labels=lab, n_labels=L, symmetric=sym, device="cuda")
    excluded = ops.pair_mask_dense(mask, N, N)
    got = ops.bilinear_ensemble_topk(z, z, ws, k, eligible=eligible, precision=prec, exclude=mask)
    _check(got, _expected(P, k, eligible, excluded))
    if planes == "shared":
        assert bool((got[1][:, 7] == -1).all()) and bool((got[0][:, 7] == NEG).all())        # a fully excluded row is all padding
    # row 200 of outcome 0: columns 41 onward of the dense order, minus the random pairs that hit the row
    # (at least 200 - 40 - a handful of eligible columns remain, so the first k of the rest are all eligible)
    gone = excluded[0, 200].cpu()
    rest = [c for c in order[0, 200, 40:].tolist() if not bool(gone[c])]
    assert got[1][0, 200].tolist() == rest[:k]


@pytest.mark.parametrize("eligible", ["all", "lower"])
def test_no_mask_and_an_all_zero_mask_agree(eligible):
    from madrigal_amd import ops
    z, _, ws, _ = _case(5, 300, 300, 2, 0.3, "bf16x3", True)
    none = ops.bilinear_ensemble_topk(z, z, ws, 16, eligible=eligible)
    for P in (1, 2):
        zero = torch.zeros((P, (300 + 31) // 32, 320), dtype=torch.int32, device="cuda")
        _check(ops.bilinear_ensemble_topk(z, z, ws, 16, eligible=eligible, exclude=zero), none)


# ---- determinism, out ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,scale", [(5, 0.3), (1, 1.0)])
def test_two_calls_agree_and_out_is_filled(K, scale):
    from madrigal_amd import ops
    zh, zt, ws, _ = _case(K, 300, 1001, 2, scale, "bf16x3", False)
    a = ops.bilinear_ensemble_topk(zh, zt, ws, 32)
    b = ops.bilinear_ensemble_topk(zh, zt, ws, 32)
    _check(b, a)
    out = (torch.full((2, 300, 32), float("nan"), device="cuda"), torch.full((2, 300, 32), -7, dtype=torch.int32, device="cuda"))
    back = ops.bilinear_ensemble_topk(zh, zt, ws, 32, out=out)
    assert back[0] is out[0] and back[1] is out[1]
    _check(out, a)
    with pytest.raises(ValueError):
        ops.bilinear_ensemble_topk(zh, zt, ws, 32, out=(out[0][:, :, :16], out[1]))
    with pytest.raises(ValueError, match="one drug set"):
        ops.bilinear_ensemble_topk(zh, zt, ws, 4, eligible="not_self")


# ---- pipeline --------------------------------------------------------------------------------------------------------------------
def _weights(K, L, seed):
    return [_rand((L, 128, 128), seed + m, 1 / np.sqrt(128)).cuda() for m in range(K)]


def test_ensemble_top_partners_rows_and_label_range():
    from madrigal_amd import models as M, ops
    from madrigal_amd.pipeline import ensemble_top_partners
    K, N, L = 3, 300, 5
    w = _weights(K, L, 40)
    zs = [_rand((N, 128), 50 + m, 0.3).cuda() for m in range(K)]
    with M.precision("bf16x3"):
        full = ensemble_top_partners(w, zs, 8)
        _check(full, _expected(_dense(zs, zs, [ops.symmetrize(t) for t in w], "bf16x3"), 8, "not_self"))
        rows = [299, 3, 150, 3, 0, 77]
        part = ensemble_top_partners(w, zs, 8, label_range=(1, 4), drug_rows=rows, max_temp_bytes=N * 8 * 8)      # one outcome per chunk
        _check(part, (full[0][1:4][:, rows], full[1][1:4][:, rows]))
        _check(ensemble_top_partners(w, zs, 8, label_range=(2, 5)), (full[0][2:5], full[1][2:5]))
        h, t = _random_pairs(N, 0.01, 9)
        known = ops.pair_mask(h, t, N, symmetric=True, device="cuda")
        _check(ensemble_top_partners(w, zs, 8, exclude=known),
               _expected(_dense(zs, zs, [ops.symmetrize(t) for t in w], "bf16x3"), 8, "not_self", ops.pair_mask_dense(known, N, N)))


def _brute_pairs(P, K, excluded=None):
    """The K best of the strict lower triangle of the dense P in the order (P descending, head ascending, tail ascending)."""
    L, N, _ = P.shape
    Q = torch.where(_allowed(N, N, "lower", P.device)[None], P, torch.full_like(P, NEG))
    if excluded is not None:
        Q = Q.masked_fill(excluded.expand(L, N, N), NEG)
    v, f = torch.sort(Q.reshape(L, N * N), dim=1, descending=True, stable=True)
    v, f = v[:, :K], f[:, :K]
    dead = v == NEG
    return v, torch.where(dead, torch.full_like(f, -1), f // N), torch.where(dead, torch.full_like(f, -1), f % N)


@pytest.mark.parametrize("K_models,scale", [(5, 0.3), (1, 1.0)])
def test_ensemble_top_pairs_equals_the_brute_force(K_models, scale):
    from madrigal_amd import models as M, ops
    from madrigal_amd.pipeline import ensemble_top_pairs
    N, L = 300, 3
    w = _weights(K_models, L, 60)
    zs = [_rand((N, 128), 70 + m, scale).cuda() for m in range(K_models)]
    P = _dense(zs, zs, [ops.symmetrize(t) for t in w], "bf16x3")
    h, t = _random_pairs(N, 0.01, 11)
    known = ops.pair_mask(h, t, N, symmetric=True, device="cuda")
    opened = 0
    with M.precision("bf16x3"):
        for K in (1, 10, 1000):
            want = _brute_pairs(P, K)
            for k_row in (1, 4, 16):
                info = {}
                got = ensemble_top_pairs(w, zs, K, k_row=k_row, info=info)
                for g, x in zip(got, want):
                    assert torch.equal(g, x), (K, k_row)
                assert len(info["open_rows"]) == L
                opened += sum(info["open_rows"])
        got = ensemble_top_pairs(w, zs, 1000, k_row=4, exclude=known, label_range=(1, 3))
        for g, x in zip(got, _brute_pairs(P[1:3], 1000, ops.pair_mask_dense(known, N, N))):
            assert torch.equal(g, x)
    assert opened > 0                                  # rows were re-scored with the dense ensemble sweep, and the result stayed exact


def test_model_level_three_checkpoints():
    """Three twosides321 checkpoints as in test_ensemble_gpu: ensemble_top_partners(models, zs, 8) is the sorted
    ensemble_all_pairs(models, zs, drug_2_inds=all) (an index list on the tail side: the general sweep), and the decoder or the
    original weight in place of the model give the same bits."""
    from madrigal_amd import configs, data as D, models as M
    from madrigal_amd.pipeline import ensemble_all_pairs, ensemble_top_partners, generate_embeddings
    from oracle.params import det_state_dict
    n, L = 40, 321
    batch, bkg = D.make_batch(n, 5, kg_nodes=300, kg_edges=2500)
    b = D.batch_to(batch, "cuda")
    kgc = {"data": bkg["data"].to("cuda"), "drug_index_map": bkg["drug_index_map"].cuda()}
    filler = _rand((n, 128), 6).cuda()
    models, zs = [], []
    for seed in (11, 12, 13):
        model = configs.build_model("twosides321", bkg["data"], L)
        sd = model.state_dict()
        skip = [k for k in sd if k.endswith("pos_encoder.pe")]
        model.load_state_dict({**sd, **det_state_dict(seed, {k: tuple(v.shape) for k, v in sd.items()}, skip)})
        model = model.cuda().eval()
        with M.precision("bf16x3"):
            zs.append(generate_embeddings(model, b, kgc, kg_filler=filler).contiguous())
        models.append(model)
    with M.precision("bf16x3"):
        dense = ensemble_all_pairs(models, zs, drug_2_inds=list(range(n))).contiguous()
        got = ensemble_top_partners(models, zs, 8)
        via_dec = ensemble_top_partners([m.decoder for m in models], zs, 8)
        via_w = ensemble_top_partners([m.decoder.parametrizations.weight.original.detach() for m in models], zs, 8)
    assert got[0].shape == (L, n, 8)
    _check(got, _expected(dense, 8, "not_self"))
    _check(via_dec, got)
    _check(via_w, got)
