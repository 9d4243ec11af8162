"""Checkpoint-ensembled DDI probabilities on the HIP path (ops.bilinear_ensemble_sigmoid, pipeline.ensemble_all_pairs) against the
reference's arithmetic (madrigal/evaluate/predict.py:358-359, 493-498), against the composed single-model kernels, and at full size."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# the head's per-entry logit bound per mode (smoke(): |d| <= a |s| + a rms), the ensemble's bound is a quarter of it (sigmoid' <= 1/4)
LOGIT_A = {"bf16x3": 1e-4, "f32": 2e-5}


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _models(K, nh, nt, L, seed, sym):
    zh = [_rand((nh, 128), seed + 10 * k) for k in range(K)]
    zt = zh if sym else [_rand((nt, 128), seed + 10 * k + 1) for k in range(K)]
    w = [_rand((L, 128, 128), seed + 10 * k + 2, 1 / np.sqrt(128)) for k in range(K)]
    return zh, zt, w


def _reference(zh, zt, w):
    """predict.py:358-359 + 493-498 in numpy: raw scores per checkpoint, float32 sigmoid, stack, mean(0); also the logits."""
    from oracle import madrigal_oracle as O
    logits = [O.bilinear_scores(a, b, c).float().numpy() for a, b, c in zip(zh, zt, w)]
    probs = [(np.float32(1) / (np.float32(1) + np.exp(-s))).astype(np.float32) for s in logits]
    return np.stack(probs).mean(0), np.stack(logits)


def _bound(logits, prec):
    a = LOGIT_A[prec]
    rms = float(np.sqrt(np.mean(np.square(logits.astype(np.float64)))))
    return 0.25 * (a * np.abs(logits).max(0) + a * rms) + 1e-6


def _cuda(ts):
    return [t.cuda() for t in ts]


def _composed(zh, zt, ws, prec):
    """K single-model launches with the sigmoid epilogue, fp32 sum in model order, one division by K (row-pitched outputs)."""
    from madrigal_amd import ops
    acc = None
    for a, b, w in zip(zh, zt, ws):
        p = ops.bilinear_allpairs(a, b, w, precision=prec, epilogue=ops.EPI_STORE_SIGMOID,
                                  out=ops.empty_scores(w.shape[0], a.shape[0], b.shape[0], a.device))
        acc = p.clone() if acc is None else acc + p
    return acc / float(len(zh))


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("K,nh,nt,L,sym", [(1, 33, 33, 3, True), (2, 1, 1, 2, True), (5, 33, 33, 4, True), (8, 1001, 1001, 2, True),
                                           (2, 4003, 4003, 1, True), (5, 777, 1001, 2, False), (8, 33, 130, 3, False),
                                           (1, 1001, 300, 2, False)])
def test_against_the_reference_arithmetic(prec, K, nh, nt, L, sym):
    from madrigal_amd import ops
    zh, zt, w = _models(K, nh, nt, L, 100 + K, sym)
    want, logits = _reference(zh, zt, w)
    zhc = _cuda(zh)
    ztc = zhc if sym else _cuda(zt)
    got = ops.bilinear_ensemble_sigmoid(zhc, ztc, [ops.symmetrize(t.cuda()) for t in w], precision=prec).cpu().numpy()
    assert got.shape == (L, nh, nt) and np.isfinite(got).all()
    assert (np.abs(got - want) <= _bound(logits, prec)).all(), float(np.abs(got - want).max())


@pytest.mark.parametrize("sym", [True, False])
def test_unsorted_duplicated_indices_match_the_reference(sym):
    """The wrapper's fancy indexing (predict.py:498): [:, outcome_inds][:, :, drug_inds][..., drug_2_inds], any order, repeats."""
    from madrigal_amd import models as M
    from madrigal_amd.pipeline import ensemble_all_pairs
    K, N, L = 3, 300, 11
    z, _, w = _models(K, N, N, L, 7, True)
    oi = [9, 2, 2, 10, 0, 5]
    di = [299, 3, 3, 150, 0, 77, 201, 201, 42]
    d2 = None if sym else [5, 5, 298, 1, 100, 100, 7]
    with M.precision("bf16x3"):
        got = ensemble_all_pairs([t.cuda() for t in w], _cuda(z), drug_inds=di, drug_2_inds=d2, outcome_inds=oi).cpu().numpy()
    zsel = [t[di] for t in z]
    z2 = zsel if sym else [t[d2] for t in z]
    want, logits = _reference(zsel, z2, [t[oi] for t in w])
    full, _ = _reference(z, z, w)                                         # the reference's own order of operations on the full tensor
    ref_idx = full[oi][:, di][:, :, di if sym else d2]
    assert np.array_equal(want, ref_idx) or np.abs(want - ref_idx).max() < 1e-6
    assert got.shape == want.shape
    assert (np.abs(got - want) <= _bound(logits, "bf16x3")).all()
    if sym:
        assert np.array_equal(got, got.transpose(0, 2, 1))


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("K,N,Nt,L,sym", [(1, 1000, 1000, 3, True), (1, 700, 513, 2, False), (2, 771, 771, 2, True), (5, 516, 516, 3, True),
                                          (5, 300, 1001, 2, False), (8, 257, 257, 1, True)])
def test_against_the_composed_single_model_kernels(prec, K, N, Nt, L, sym):
    """K bilinear_allpairs(EPI_STORE_SIGMOID) launches summed in model order and divided by K, on the head's general sweep (the MFMA
    chain the ensemble reuses): within 1e-6, and bit for bit at K = 1.  Symmetric inputs: every entry is computed in ONE association
    order (z_i W z_j for the entries the sweep computes, z_j W z_i for the mirrored ones), so each entry matches ``composed[i, j]`` or
    ``composed[j, i]``.  The single-model symmetric sweep computes its 256 x 256 diagonal blocks in both orders (they differ at the
    mode's rounding of T, up to ~1e-4 of a probability in bf16x3) and runs 16x16x32 products in bf16x3 (fp32 grouping: the head's own
    tests allow 2e-6 between its two sweeps); against it each entry agrees in one of the two orders to 2e-6."""
    from madrigal_amd import ops
    zh, zt, w = _models(K, N, Nt, L, 300 + K, sym)
    zhc = _cuda(zh)
    ztc = zhc if sym else _cuda(zt)
    ws = [ops.symmetrize(t.cuda()) for t in w]
    got = ops.bilinear_ensemble_sigmoid(zhc, ztc, ws, precision=prec)
    ref = _composed(zhc, [t.clone() for t in ztc] if sym else ztc, ws, prec)      # a copy: the general sweep
    d = (got - ref).abs()
    if sym:
        d = torch.minimum(d, (got - ref.transpose(1, 2)).abs())
        ref_sym = _composed(zhc, ztc, ws, prec)                                   # the single-model symmetric sweep
        assert float(torch.minimum((got - ref_sym).abs(), (got - ref_sym.transpose(1, 2)).abs()).max()) <= 2e-6
    assert float(d.max()) <= 1e-6
    if K == 1:
        assert torch.equal(d, torch.zeros_like(d))                                # the same MFMA chain and epilogue: same bits


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("K,N", [(1, 1001), (3, 1000), (5, 300), (2, 4)])
def test_symmetric_sweep_is_exactly_symmetric(prec, K, N):
    """drug_2_inds=None: every P[l] == P[l].T bit for bit (diagonal blocks included), and within the bound of the general sweep on
    the same inputs (a copy of z on the tail side is not "the same matrix")."""
    from madrigal_amd import ops
    z, _, w = _models(K, N, N, 3, 500 + K, True)
    zc = _cuda(z)
    ws = [ops.symmetrize(t.cuda()) for t in w]
    out = ops.empty_scores(3, N, N, "cuda")
    out.fill_(float("nan"))
    sym = ops.bilinear_ensemble_sigmoid(zc, zc, ws, precision=prec, out=out)
    assert sym is out and not bool(torch.isnan(sym).any())
    assert torch.equal(sym, sym.transpose(1, 2))
    gen = ops.bilinear_ensemble_sigmoid(zc, [t.clone() for t in zc], ws, precision=prec)
    _, logits = _reference(z, z, w)
    assert (np.abs(sym.cpu().numpy() - gen.cpu().numpy()) <= _bound(logits, prec)).all()


def test_contiguous_and_pitched_destinations_agree():
    """An unpadded contiguous [L,N,N] with N % 4 != 0 (rows at any 4-byte alignment) gets the same bits as the row-pitched layout."""
    from madrigal_amd import ops
    z, zt, w = _models(3, 301, 257, 2, 900, False)
    zc, ztc, ws = _cuda(z), _cuda(zt), [ops.symmetrize(t.cuda()) for t in w]
    for tails in (zc, ztc):
        pit = ops.bilinear_ensemble_sigmoid(zc, tails, ws)
        dense = torch.full((2, 301, tails[0].shape[0]), float("nan"), device="cuda")
        assert ops.bilinear_ensemble_sigmoid(zc, tails, ws, out=dense) is dense
        assert torch.equal(dense, pit)


def test_full_size_one_launch_into_hbm():
    """K = 5 checkpoints, 4096 drugs x 896 outcomes, bf16x3, one launch into 60 GB of HBM: 32 sampled 128 x 128 blocks against the
    composed path, and no per-model score tensor (peak allocation grows by the output plus at most 1 GiB)."""
    from madrigal_amd import ops
    K, N, L = 5, 4096, 896
    free, _ = torch.cuda.mem_get_info()
    if free < 66 * 2 ** 30:
        pytest.skip("needs 66 GB of free HBM")
    zc = [_rand((N, 128), 40 + k).cuda() for k in range(K)]
    ws = [ops.symmetrize(_rand((L, 128, 128), 50 + k, 1 / np.sqrt(128)).cuda()) for k in range(K)]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    out = ops.bilinear_ensemble_sigmoid(zc, zc, ws, precision="bf16x3")
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    out_bytes = out.untyped_storage().nbytes()
    assert grown <= out_bytes + 2 ** 30, (grown, out_bytes)
    g = torch.Generator().manual_seed(3)
    starts = [0, N - 128] + [int(x) for x in torch.randint(0, N - 128, (30,), generator=g)]
    for b in range(32):
        i0, j0 = starts[b], starts[(b * 7 + 3) % 32]
        ls = torch.randint(0, L, (4,), generator=g).tolist() + [0, L - 1]
        blk = out[ls, i0:i0 + 128, j0:j0 + 128]
        rows, cols = [z[i0:i0 + 128].contiguous() for z in zc], [z[j0:j0 + 128].contiguous() for z in zc]
        wl = [w[ls].contiguous() for w in ws]
        ref = _composed(rows, cols, wl, "bf16x3")                                   # head rows i, tail columns j
        ref_t = _composed(cols, rows, wl, "bf16x3").transpose(1, 2)                 # the other association order (mirrored entries)
        d = torch.minimum((blk - ref).abs(), (blk - ref_t).abs())
        assert float(d.max()) <= 1e-6, (i0, j0)
    assert torch.equal(out[L - 1], out[L - 1].T)


@pytest.mark.parametrize("sym", [True, False])
def test_memmap_destination_equals_hbm_result(tmp_path, sym):
    """Host destination: outcome chunks of host_chunk through two pinned buffers, several chunks and a ragged last one: same bits."""
    from madrigal_amd import models as M
    from madrigal_amd.pipeline import ensemble_all_pairs
    K, N, L = 3, 260, 41
    z, _, w = _models(K, N, N, L, 21, True)
    wc, zc = [t.cuda() for t in w], _cuda(z)
    d2 = None if sym else list(range(N - 1, -1, -2))
    with M.precision("bf16x3"):
        dense = ensemble_all_pairs(wc, zc, drug_2_inds=d2)
        path = os.path.join(tmp_path, "probs.mmap")
        mm = np.memmap(path, dtype=np.float32, mode="w+", shape=tuple(dense.shape))
        got = ensemble_all_pairs(wc, zc, drug_2_inds=d2, out=mm, host_chunk=16)
        mm.flush()
    assert got is mm
    back = np.memmap(path, dtype=np.float32, mode="r", shape=tuple(dense.shape))
    assert np.array_equal(np.asarray(back), dense.cpu().numpy())
    with pytest.raises(ValueError):
        ensemble_all_pairs(wc, zc, drug_2_inds=d2, out=np.zeros((L, N, N + 1), dtype=np.float32))


def test_model_level_against_the_composed_single_model_path():
    """Three twosides321 checkpoints (different parameter seeds): pipeline.generate_embeddings per checkpoint, then
    ensemble_all_pairs(models, zs) == mean_k sigmoid(score_all_pairs(model_k, z_k)) within the bound; the decoder and the original
    weight are accepted in place of the model with the same bits."""
    from madrigal_amd import configs, data as D, models as M
    from madrigal_amd.pipeline import ensemble_all_pairs, generate_embeddings, score_all_pairs
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
        got = ensemble_all_pairs(models, zs)
        logits = [score_all_pairs(m, z) for m, z in zip(models, zs)]
        via_dec = ensemble_all_pairs([m.decoder for m in models], zs)
        via_w = ensemble_all_pairs([m.decoder.parametrizations.weight.original.detach() for m in models], zs)
    comp = sum(torch.sigmoid(s) for s in logits) / 3.0
    lg = torch.stack(logits).cpu().numpy()
    assert got.shape == (L, n, n)
    assert (np.abs(got.cpu().numpy() - comp.cpu().numpy()) <= _bound(lg, "bf16x3")).all()
    assert torch.equal(via_dec, got) and torch.equal(via_w, got)
