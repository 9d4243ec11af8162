"""GPU checks of the grouped metrics and the drug-stratified evaluation (csrc/eval_metrics.hip mdg_group_metrics -> ops.group_metrics
-> metrics.drug_specific_metrics -> predict.get_drug_specific_scores) against the sklearn restatements of test_eval_metrics_cpu /
test_drug_metrics_cpu and the reference's recorded outputs (tests/golden/drug_metrics.npz)."""
import os

import numpy as np
import pytest
import torch

from test_drug_metrics_cpu import check_values, golden_cases, restate_drug_scores
from test_eval_metrics_cpu import restate_binary

pytestmark = pytest.mark.gpu
WALKS = ("0", "1", "3")                                            # by size, every group by one thread, every group by a workgroup


class walk_setting:
    """MDG_GROUP_WALK for the duration of a block (the library re-reads its switches after mdg_tuning_reload)."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from madrigal_amd._lib import lib
        self.old = os.environ.get("MDG_GROUP_WALK")
        os.environ["MDG_GROUP_WALK"] = self.value
        lib().mdg_tuning_reload()

    def __exit__(self, *exc):
        from madrigal_amd._lib import lib
        if self.old is None:
            os.environ.pop("MDG_GROUP_WALK", None)
        else:
            os.environ["MDG_GROUP_WALK"] = self.old
        lib().mdg_tuning_reload()


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _sparse_case(seed, sizes, quant=32):
    """Groups of the given sizes under sparse ids (0 and 2^31 - 1 included), shuffled; scores quantised (heavy ties)."""
    rng = np.random.default_rng(seed)
    ids = np.unique(np.concatenate([[0, 2 ** 31 - 1], rng.integers(1, 2 ** 31 - 1, 4 * len(sizes))]))
    ids = rng.permutation(ids)[:len(sizes)]
    ids[0], ids[1] = 0, 2 ** 31 - 1
    group = np.repeat(ids, sizes).astype(np.int64)
    perm = rng.permutation(group.size)
    group = group[perm]
    rate = rng.uniform(0.1, 0.7, len(sizes))
    ys = (rng.random(group.size) < np.repeat(rate, sizes)[perm]).astype(np.float32)
    preds = np.clip(0.3 * ys + 0.7 * rng.random(group.size), 0, 1)
    preds = (np.round(preds * quant) / quant).astype(np.float32)
    return preds, ys, group


SIZES_INT = [1, 2, 3, 33, 2049, 100_000] + list(np.random.default_rng(7).integers(1, 40, 200))
SIZES_FRAC = [4, 33, 2049, 100_000] + list(np.random.default_rng(8).integers(4, 40, 120))


def _restate_groups(preds, ys, group, k):
    want = {}
    for g in np.unique(group):
        m = group == g
        want[int(g)] = restate_binary(preds[m], ys[m], k) + (int(m.sum()), float(ys[m].sum()))
    return want


@pytest.mark.parametrize("k, sizes, seed", [(50, SIZES_INT, 1), (0.25, SIZES_FRAC, 2)])
def test_group_metrics_against_the_restatement_under_every_walk(k, sizes, seed):
    from madrigal_amd import ops
    preds, ys, group = _sparse_case(seed, sizes)
    want = _restate_groups(preds, ys, group, k)
    first = None
    for w in WALKS:
        with walk_setting(w):
            r = ops.group_metrics(*_dev(preds, ys, group), 2 ** 31, k=k)
        gid, cnt, pos, keff = (r[x].cpu().numpy() for x in ("group_id", "count", "pos", "k_eff"))
        vals = r["values"].cpu().numpy()
        np.testing.assert_array_equal(gid, np.array(sorted(want)))
        for j, g in enumerate(gid):
            v, kk, n, p = want[int(g)]
            assert (cnt[j], pos[j], keff[j]) == (n, p, kk), (w, g)
            _check(vals[:, j], v, f"walk {w} group {g} (n = {n})")
        if first is None:
            first = (gid, cnt, pos, keff)
        else:
            for a, b in zip(first, (gid, cnt, pos, keff)):
                np.testing.assert_array_equal(a, b)


def _check(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    f32 = np.zeros(13, dtype=bool)
    f32[7:9] = True
    np.testing.assert_allclose(got[~f32], want[~f32], rtol=1e-10, atol=1e-15, equal_nan=True, err_msg=what)
    np.testing.assert_allclose(got[f32], want[f32], rtol=1e-6, atol=0, equal_nan=True, err_msg=what)


def test_two_calls_are_bitwise_equal():
    from madrigal_amd import data as D, ops
    lab, h, t, pn = D.make_eval_triples(512, 512, 64, 60_000, 4)
    g = torch.Generator().manual_seed(3)
    pred = torch.sigmoid(2 * pn - 1 + torch.randn(pn.numel(), generator=g))
    group = (h * 64 + lab).cuda()
    args = (pred.cuda(), pn.cuda(), group, 512 * 64)
    a = ops.group_metrics(*args, k=0.5, inner=64)                 # groups of 3 or more: k resolves to 1 at least
    b = ops.group_metrics(*args, k=0.5, inner=64)
    assert a.keys() == b.keys() and len(a) == 7
    for key in a:
        x, y = a[key].contiguous(), b[key].contiguous()
        assert torch.equal(x.view(torch.int64), y.view(torch.int64)), key


def test_workgroup_walk_on_labels_matches_label_metrics_bit_for_bit():
    from madrigal_amd import ops
    from test_eval_metrics_gpu import _zipf_case
    preds, ys, labels = _zipf_case(300_000, 896, 9)
    args = _dev(preds, ys, labels)
    ref = ops.label_metrics(*args, 896, k=50)
    with walk_setting("3"):
        r = ops.group_metrics(*args, 896, k=50)
    gid = r["group_id"].cpu().numpy()
    np.testing.assert_array_equal(gid, np.flatnonzero(ref["count"].cpu().numpy() > 0))
    want = ref["values"][:, r["group_id"]].contiguous()
    assert torch.equal(r["values"].contiguous().view(torch.int64), want.view(torch.int64))
    for key in ("count", "pos", "k_eff"):
        assert torch.equal(r[key], ref[key][r["group_id"]]), key


@pytest.mark.parametrize("walk", WALKS)
def test_outer_means_are_numpy_means_of_the_group_values(walk):
    from madrigal_amd import data as D, ops
    L, n_drugs = 40, 300
    lab, h, t, pn = D.make_eval_triples(n_drugs, 500, L, 20_000, 6)
    g = torch.Generator().manual_seed(5)
    pred = torch.sigmoid(2 * pn - 1 + torch.randn(pn.numel(), generator=g))
    keep = h != 17                                                   # an outer index without groups
    group = (h * L + lab)[keep]
    with walk_setting(walk):
        r = ops.group_metrics(pred[keep].cuda(), pn[keep].cuda(), group.cuda(), n_drugs * L + 5, k=50, inner=L)
    vals, gid = r["values"].cpu().numpy(), r["group_id"].cpu().numpy()
    ov, og = r["outer_values"].cpu().numpy(), r["outer_groups"].cpu().numpy()
    assert ov.shape == (13, n_drugs + 1) and og.shape == (n_drugs + 1,)
    for o in range(n_drugs + 1):
        sel = np.flatnonzero(gid // L == o)
        assert og[o] == sel.size
        if sel.size == 0:
            assert np.isnan(ov[:, o]).all() and o in (17, n_drugs)
            continue
        want = np.ascontiguousarray(vals[:, sel].T).mean(axis=0)
        fin = ~np.isnan(want)                                        # bit-equal where finite, NaN where numpy gives NaN
        np.testing.assert_array_equal(np.isnan(ov[:, o]), ~fin, err_msg=f"outer {o}")
        np.testing.assert_array_equal(ov[fin, o].view(np.int64), want[fin].view(np.int64), err_msg=f"outer {o}")


def test_drug_specific_metrics_against_the_reference_golden():
    from madrigal_amd import metrics
    n = 0
    for name, mode, n_head, n_tail, preds, heads, tails, labels, pos_neg, want in golden_cases():
        args = _dev(preds, heads, tails, labels, pos_neg)
        if "exception" in want:
            with pytest.raises(ValueError, match="drug"):
                metrics.drug_specific_metrics(*args, n_head, mode)
            continue
        got, owners = metrics.drug_specific_metrics(*args, n_head, mode)
        assert list(got.keys()) == want["names"], name
        offset = 10_000 if mode == "test_between" else 20_000
        np.testing.assert_array_equal(owners + offset, want["drugs"], err_msg=name)
        vals = np.array([got[nm] for nm in want["names"]])
        assert all(isinstance(v, np.float64) for v in got["auprc"])
        check_values(vals, want["values"], name, rtol=1e-10)
        n += 1
    assert n == 4


def test_drug_specific_metrics_error_paths():
    from madrigal_amd import metrics, ops
    lab, h, t, pn = (x.numpy() for x in __import__("madrigal_amd.data", fromlist=["x"]).make_eval_triples(10, 12, 4, 40, 1))
    p = np.linspace(0.01, 0.99, pn.size).astype(np.float32)
    args = _dev(p, h, t, lab, pn)
    metrics.drug_specific_metrics(*args, 10, "test_between")
    with pytest.raises(ValueError, match="drug 10: no positive"):       # head drug 10 of 11 has none
        metrics.drug_specific_metrics(*args, 11, "test_between")
    with pytest.raises(ValueError, match="lack negatives"):
        metrics.drug_specific_metrics(*(a[:-3] for a in args), 10, "test_between")
    with pytest.raises(ValueError, match="CUDA"):
        metrics.drug_specific_metrics(args[0].cpu(), *args[1:], 10, "test_between")
    lab1 = lab.copy()
    lab1[40] = 4                                                        # a lone negative under a new label, pred < 0.5
    p1 = p.copy()
    p1[40] = 0.2
    with pytest.raises(ValueError, match=f"drug {h[0]}, label 4: .*one class"):
        metrics.drug_specific_metrics(*_dev(p1, h, t, lab1, pn), 10, "test_between")
    y = torch.tensor([0.0, 1.0, 1.0, 0.0]).cuda()
    g = torch.tensor([0, 0, 3, 3]).cuda()
    pr = torch.tensor([0.2, 0.7, 0.9, 0.4]).cuda()
    with pytest.raises(ValueError, match="NaN"):
        ops.group_metrics(torch.tensor([0.2, float("nan"), 0.9, 0.4]).cuda(), y, g, 4)
    with pytest.raises(ValueError, match="group id"):
        ops.group_metrics(pr, y, g, 3)
    with pytest.raises(ValueError, match="target"):
        ops.group_metrics(pr, y * 2, g, 4)
    with pytest.raises(ValueError, match="resolves to 0"):
        ops.group_metrics(pr, y, g, 4, k=0.1)
    with pytest.raises(ValueError, match="GPU"):
        ops.group_metrics(pr.cpu(), y, g, 4)
    with pytest.raises(ValueError, match="n_groups"):
        ops.group_metrics(pr, y, g, 2 ** 31 + 1)


def test_get_drug_specific_scores_end_to_end_on_a_small_model():
    from madrigal_amd import configs, data as D, masks as MK, models as M, predict
    n, L, seed = 64, 6, 13
    batch, bkg = D.make_batch(n, seed, kg_nodes=300, kg_edges=2500)
    torch.manual_seed(seed)
    model = configs.build_model("drugbank163", bkg["data"], L).cuda().eval()
    lab, h, t, pn = D.make_eval_triples(n, n, L, 300, seed)
    full = {"head": batch, "tail": batch, "kg": bkg, "edge_indices": {"head": h, "tail": t, "label": lab, "pos_neg": pn}}
    filler = torch.randn(n, 128, generator=torch.Generator().manual_seed(1)).cuda()
    ft_mode = "str_str+random_sample"
    with M.precision("f32"):
        pred = predict.make_predictions(model, full, "full_full", ft_mode, "cuda", kg_filler=filler)
        dense = predict.make_predictions(model, full, "full_full", ft_mode, "cuda", return_all_pairwise=True, kg_filler=filler)
        got, drugs = predict.get_drug_specific_scores(model, full, "full_full", ft_mode, "cuda", kg_filler=filler)
        got_t, drugs_t = predict.get_drug_specific_scores(model, full, "full_full", ft_mode, "cuda", mode="test_between_train",
                                                          kg_filler=filler)
    assert pred.device.type == "cpu" and dense.shape == (L, n, n)
    gathered = dense[lab, h, t]
    assert float((pred - gathered).abs().max()) < 2e-5
    for mode, res, dr in (("test_between", got, drugs), ("test_between_train", got_t, drugs_t)):
        names, want, idx = restate_drug_scores(gathered.numpy(), h.numpy(), t.numpy(), lab.numpy(), pn.numpy(), n, mode)
        assert list(res.keys()) == names
        assert torch.equal(dr, batch["drugs"][torch.from_numpy(idx)])
        check_values(np.array([res[nm] for nm in names]), want, mode, rtol=1e-10)
