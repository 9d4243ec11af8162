"""GPU checks of the evaluation metrics (csrc/eval_metrics.hip -> ops.label_metrics -> metrics.get_metrics -> evaluate.evaluate_ddi)
against the reference's recorded outputs (tests/golden/eval_metrics.npz) and the sklearn restatement of test_eval_metrics_cpu."""
import numpy as np
import pytest
import torch

from test_eval_metrics_cpu import golden_runs, restate_binary

pytestmark = pytest.mark.gpu
F32_AT_K = np.zeros(13, dtype=bool)
F32_AT_K[7:9] = True                                               # recall@k, precision@k: float32 arithmetic in the reference


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    rows = F32_AT_K if got.shape[0] == 13 else np.zeros(got.shape[0], bool)
    np.testing.assert_allclose(got[~rows], want[~rows], rtol=1e-10, atol=1e-15, equal_nan=True, err_msg=what)
    np.testing.assert_allclose(got[rows], want[rows], rtol=1e-6, atol=0, equal_nan=True, err_msg=what)


def _check_labels(r, preds, ys, labels, k, which):
    vals, cnt = r["values"].cpu().numpy(), r["count"].cpu().numpy()
    for l in which:
        m = labels == l
        assert cnt[l] == m.sum()
        if not m.any():
            assert np.isnan(vals[:, l]).all()
            continue
        want, kk = restate_binary(preds[m], ys[m], k)
        assert int(r["k_eff"][l]) == kk
        _close(vals[:, l], want, f"label {l}")


def _zipf_case(T, L, seed, quant=64):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, L + 1) ** 1.1
    labels = rng.choice(L, size=T, p=w / w.sum())
    labels[:40] = np.arange(L - 40, L)                              # 1-triple labels (the rarest ones hold few or none)
    ys = (rng.random(T) < 0.3).astype(np.float32)
    preds = np.clip(0.3 * ys + 0.7 * rng.random(T), 0, 1)
    preds = (np.round(preds * quant) / quant).astype(np.float32)     # heavy ties: 65 distinct scores
    preds[rng.random(T) < 0.03] = 1.0
    return preds, ys, labels.astype(np.int64)


def _dev(*arrs):
    return [torch.from_numpy(a).cuda() for a in arrs]


def test_golden_cases_through_get_metrics():
    from madrigal_amd import metrics
    n = 0
    for name, task, avg, k, preds, ys, labels, want_names, want, want_pos in golden_runs():
        d, pos = metrics.get_metrics(preds, ys, labels, k=k, task=task, average=avg, verbose=False)
        assert list(d.keys()) == want_names, (name, avg)
        _close(np.array(list(d.values())), want, f"{name}/{task}/{avg}")
        np.testing.assert_array_equal(np.asarray(pos, np.float64), want_pos)
        n += 1
    assert n == 9


def test_random_zipf_labels_with_ties_against_the_restatement():
    from madrigal_amd import ops
    preds, ys, labels = _zipf_case(200_000, 896, 3)
    for k in (50, 0.25):
        r = ops.label_metrics(*_dev(preds, ys, labels), 896, k=k)
        _check_labels(r, preds, ys, labels, k, range(896))


def test_top_k_boundary_inside_a_tie_group_follows_the_stable_rule():
    from madrigal_amd import ops
    rng = np.random.default_rng(5)
    n = 400
    preds = np.full(n, 0.75, np.float32)
    preds[:30] = 0.9                                                 # 30 above, then a run of 370 ties across k = 50
    preds[200:] = rng.random(200).astype(np.float32) * 0.5
    ys = (rng.random(n) < 0.5).astype(np.float32)
    labels = np.zeros(n, np.int64)
    order = np.argsort(preds, kind="stable")[::-1]
    r = ops.label_metrics(*_dev(preds, ys, labels), 1, k=50)
    top = order[:50]
    v = r["values"].cpu().numpy()[:, 0]
    y64 = ys.astype(np.float64)
    assert v[8] == y64[top].sum() / 50 and v[7] == y64[top].sum() / y64.sum()
    _check_labels(r, preds, ys, labels, 50, [0])


def test_one_huge_label_beside_hundreds_of_small_ones():
    from madrigal_amd import ops
    rng = np.random.default_rng(11)
    big, L = 3_100_000, 400
    labels = np.concatenate([np.full(big, 7), rng.integers(0, L, 60_000)])
    rng.shuffle(labels)
    T = labels.size
    ys = (rng.random(T) < 0.2).astype(np.float32)
    preds = np.clip(0.25 * ys + 0.75 * rng.random(T), 0, 1).astype(np.float32)
    preds = (np.round(preds * 4096) / 4096).astype(np.float32)
    r = ops.label_metrics(*_dev(preds, ys, labels.astype(np.int64)), L, k=1000)
    _check_labels(r, preds, ys, labels, 1000, [7] + list(range(0, L, 37)))


def test_full_size_sampled_labels_and_macro_auprc():
    from madrigal_amd import data as D, metrics as MT, ops
    lab, hd, tl, y = D.make_labelled_triples(4096, 896, 1_000_000, 21)
    T = lab.numel()
    assert T == 6_000_000
    g = torch.Generator().manual_seed(2)
    pred = torch.sigmoid(2.0 * y - 1.0 + torch.randn(T, generator=g))
    r = ops.label_metrics(pred.cuda(), y.cuda(), lab.cuda(), 896, k=50)
    p, yy, ll = pred.numpy(), y.numpy(), lab.numpy()
    _check_labels(r, p, yy, ll, 50, np.random.default_rng(0).choice(896, 64, replace=False))
    macro, per = MT.macro_auprc(pred.cuda(), y.cuda(), lab.cuda(), 896)
    pos, cnt = r["pos"].cpu().numpy(), r["count"].cpu().numpy()
    assert ((pos > 0) & (pos < cnt)).all()
    mine = r["values"][3].cpu().numpy()
    np.testing.assert_allclose(mine, per.cpu().numpy(), rtol=1e-12, atol=0)
    assert abs(float(np.mean(mine)) - float(macro)) < 1e-12


def test_two_calls_are_bitwise_equal():
    from madrigal_amd import ops
    preds, ys, labels = _zipf_case(300_000, 896, 9)
    args = _dev(preds, ys, labels)
    a = ops.label_metrics(*args, 896, k=0.1)
    b = ops.label_metrics(*args, 896, k=0.1)
    for key in ("values", "count", "pos", "k_eff"):
        assert torch.equal(a[key].view(torch.int64), b[key].view(torch.int64)), key


def test_value_errors():
    from madrigal_amd import metrics, ops
    p, y, l = _dev(np.array([0.2, 0.7, 0.9, 0.4], np.float32), np.array([0, 1, 1, 0], np.float32), np.array([0, 0, 1, 1], np.int64))
    bad_p = p.clone()
    bad_p[1] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        ops.label_metrics(bad_p, y, l, 2)
    bad_p[1] = float("inf")
    with pytest.raises(ValueError, match="NaN or infinite"):
        ops.label_metrics(bad_p, y, l, 2)
    with pytest.raises(ValueError, match="label"):
        ops.label_metrics(p, y, l, 1)
    with pytest.raises(ValueError, match="target"):
        ops.label_metrics(p, y * 2, l, 2)
    with pytest.raises(ValueError, match="resolves to 0"):
        ops.label_metrics(p, y, l, 2, k=0.1)
    with pytest.raises(ValueError, match="GPU"):
        ops.label_metrics(p.cpu(), y, l, 2)
    with pytest.raises(ValueError, match="one class"):                 # the reference's confusion_matrix unpack fails
        metrics.get_metrics(np.array([0.1, 0.2, 0.9, 0.8], np.float32), np.array([0, 0, 1, 1], np.float32), np.array([0, 0, 1, 1]),
                            verbose=False)


@pytest.mark.parametrize("split, eval_type", [("train", "full_full"), ("val", "str_full"), ("test_between", "full_full")])
def test_evaluate_ddi_on_the_small_model(split, eval_type):
    from madrigal_amd import data as D, masks as MK, models as M
    from madrigal_amd.evaluate import evaluate_ddi
    from test_eval_metrics_cpu import restate_get_metrics
    from test_train_gpu import _small_model
    case = ("drugbank163", "transformer", 4, "learnable", 8, 64, 256, 2, True, "x-attn", True, False)
    n, L, seed = 96, 8, 41
    model, _, batch, bkg, masks = _small_model(M, case, n, L, seed, default_init=True)     # logits of order one
    model = model.cuda().eval()
    b = D.batch_to(batch, "cuda")
    kgc = {"data": bkg["data"].to("cuda"), "drug_index_map": bkg["drug_index_map"].cuda()}
    filler = torch.randn(n, 128, generator=torch.Generator().manual_seed(1)).cuda()
    lab, hd, tl, y = D.make_labelled_triples(n, L, 400, seed)
    # the restated direction rules (evaluate.py:161-187)
    if split == "train":
        keep = hd < tl
        want = (hd[keep], tl[keep], lab[keep], y[keep])
    elif split == "val":
        want = (torch.cat([hd, tl]), torch.cat([tl, hd]), lab.repeat(2), y.repeat(2))
    else:
        want = (hd, tl, lab, y)
    best = {}
    ft_mode = "str_str+random_sample"
    with M.precision("f32"):
        key, d, loss, got = evaluate_ddi(model, b, b, kgc, masks, masks, hd, tl, lab, y, torch.nn.BCELoss(), 50, "multilabel", eval_type,
                                         split, ft_mode, best, verbose=False, return_all=True, kg_filler=filler)
        mh, mt = MK.get_evaluate_masks(masks, masks, eval_type, ft_mode, "cuda")
        with torch.no_grad():
            dense = torch.sigmoid(model(b, b, mh, mt, kgc, kg_filler=filler)).cpu()
    for nm, w in zip(("heads", "tails", "labels", "targets"), want):
        assert torch.equal(got[nm].cpu(), w.to(got[nm].dtype)), nm
    pred = got["pred"].cpu()
    ref_pred = dense[want[2], want[0], want[1]]
    assert float((pred - ref_pred).abs().max()) < 2e-5
    names, vals, _ = restate_get_metrics(pred.numpy(), want[3].numpy(), want[2].numpy(), k=50)
    assert list(d.keys()) == names and key == d["auprc"]
    _close(np.array(list(d.values())), vals, f"{split}/{eval_type}")
    loss_cpu = float(torch.nn.BCELoss()(pred, want[3]))
    assert abs(loss - loss_cpu) <= 1e-6 * max(1.0, abs(loss_cpu))
    assert set(best) == {f"best_{split}_{eval_type}_{nm}" for nm in names}
    with pytest.raises(NotImplementedError):
        evaluate_ddi(model, b, b, kgc, masks, masks, hd, tl, lab, y, torch.nn.BCELoss(), 50, "multilabel", eval_type, split, ft_mode, None,
                     verbose=False, data_source="ONSIDES", kg_filler=filler)
